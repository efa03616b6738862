"""The device memory one search of a local-search batch context takes (csrc/local_ctx.c: nla_local_ctx_bytes_per_search, what
nlopt_amd_optimize_batch sizes its chunks from), against an independent statement of the layout: the formula below is written from the
public sizing functions of include/nlopt_amd.h and the sizes of the two records only, for every algorithm (0 LD_LBFGS, 1 LD_MMA,
2 LN_COBYLA), kind of objective, both sides of the LDS kernel's limit (n = 51 / 52) and of NLA_COBYLA_GLOBAL_MAX_N (256 / 257).

Counted: the rows X, the results, and for an objective evaluated outside the kernel the request records, EX, EG (LN_COBYLA never asks for
a gradient: none), EF, the waiting list and the coroutine's saved state; then the algorithm's workspaces.  Not counted: pinned host
memory and LN_COBYLA's fixed 8-double gradient token.  A launcher the loaded device layer does not have (the emulated layer has neither
the global-memory nor the coroutine COBYLA) contributes nothing: such contexts are never created there.

Once over the emulated device layer on the CPU, once (marked gpu) over the product library; nothing is launched."""
import ctypes as C
import os

import pytest

import nlopt_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "oracle", "libnlopt_amd_emu.so")
DEVICE, HOST, USER = 0, 1, 2
LBFGS, MMA, COBYLA = 0, 1, 2
GLOBAL_MAX_N = 256                    # NLA_COBYLA_GLOBAL_MAX_N


class Evaluator(C.Structure):         # nla_evaluator (csrc/nla_internal.h); the function under test reads `kind` only
    _fields_ = [("kind", C.c_int), ("obj", C.c_int), ("f", C.c_void_p), ("f_data", C.c_void_p), ("user", C.c_void_p), ("sign", C.c_double)]


class Result(C.Structure):            # nla_lbfgs_result
    _fields_ = [("f", C.c_double), ("ret", C.c_int32), ("nevals", C.c_int32), ("iterm", C.c_int32), ("cols", C.c_int32)]


class Req(C.Structure):               # nla_local_req
    _fields_ = [("state", C.c_int32), ("want_grad", C.c_int32)]


def _fn(L, name, args):
    try:
        f = getattr(L, name)
    except AttributeError:
        return None
    f.restype, f.argtypes = C.c_size_t, [C.c_int] * args
    return f


def bind(L):
    S = {nm: _fn(L, nm, k) for nm, k in (("nla_lbfgs_work_doubles", 3), ("nla_lbfgs_hist_doubles", 3), ("nla_lbfgs_save_bytes", 0),
                                          ("nla_mma_work_doubles", 2), ("nla_mma_save_bytes", 0), ("nla_cobyla_work_doubles", 3),
                                          ("nla_cobyla_work_ints", 2), ("nla_cobyla_global_work_doubles", 2),
                                          ("nla_cobyla_ext_work_doubles", 2), ("nla_cobyla_save_bytes", 1))}
    S["has_global"] = hasattr(L, "nla_k_cobyla_batch_global") and S["nla_cobyla_global_work_doubles"] is not None
    S["has_ext"] = hasattr(L, "nla_k_cobyla_batch_ext") and S["nla_cobyla_ext_work_doubles"] is not None and S["nla_cobyla_save_bytes"] is not None
    L.nla_cobyla_fits.restype, L.nla_cobyla_fits.argtypes = C.c_int, [C.c_int]
    L.nla_local_ctx_bytes_per_search.restype = C.c_size_t
    L.nla_local_ctx_bytes_per_search.argtypes = [C.c_int, C.POINTER(Evaluator), C.c_int, C.c_int]
    return L, S


def expected(L, S, alg, kind, n, mf):
    ld = (n + 1) & ~1
    b = 8 * ld + C.sizeof(Result)
    if kind != DEVICE:
        save = {LBFGS: S["nla_lbfgs_save_bytes"](), MMA: S["nla_mma_save_bytes"](), COBYLA: S["nla_cobyla_save_bytes"](n) if S["has_ext"] else 0}[alg]
        b += C.sizeof(Req) + 8 * (ld + (0 if alg == COBYLA else ld) + 1) + 4 + save
    if alg == COBYLA:
        if kind == USER:
            work = S["nla_cobyla_ext_work_doubles"](n, 1) if S["has_ext"] else 0
        elif L.nla_cobyla_fits(n) or not (S["has_global"] and 1 <= n <= GLOBAL_MAX_N):
            work = S["nla_cobyla_work_doubles"](n, ld, 1)
        else:
            work = S["nla_cobyla_global_work_doubles"](n, 1)
        b += 8 * work + 4 * S["nla_cobyla_work_ints"](n, 1)
    elif alg == MMA:
        b += 8 * S["nla_mma_work_doubles"](ld, 1)
    else:
        b += 8 * (S["nla_lbfgs_work_doubles"](ld, mf, 1) + S["nla_lbfgs_hist_doubles"](ld, mf, 1)) + 4 * ld
    return b


GRID = [(alg, kind, n, mf) for alg in (LBFGS, MMA, COBYLA) for kind in (DEVICE, HOST, USER) for n in (1, 2, 7, 51, 52, 64, 256, 257) for mf in (1, 10)]


def check(L, S, alg, kind, n, mf):
    ev = Evaluator(kind=kind, sign=1.0)
    want, got = expected(L, S, alg, kind, n, mf), L.nla_local_ctx_bytes_per_search(alg, C.byref(ev), n, mf)
    print("alg %d kind %d n %d mf %d: %d bytes per search, the layout says %d" % (alg, kind, n, mf, got, want))
    assert got == want and got > 0


@pytest.fixture(scope="module")
def emu():
    assert os.path.exists(EMU), "oracle/libnlopt_amd_emu.so is not built (build() makes it)"
    return bind(C.CDLL(EMU))


@pytest.fixture(scope="module")
def product():
    return bind(nlopt_amd.lib())


@pytest.mark.parametrize("alg,kind,n,mf", GRID)
def test_bytes_per_search_is_the_layout_on_the_emulated_device_layer(emu, alg, kind, n, mf):
    L, S = emu
    assert not S["has_global"] and not S["has_ext"]          # (what makes this the other side of the weak references)
    check(L, S, alg, kind, n, mf)


@pytest.mark.gpu
@pytest.mark.parametrize("alg,kind,n,mf", GRID)
def test_bytes_per_search_is_the_layout_in_the_product_library(product, alg, kind, n, mf):
    L, S = product
    assert S["has_global"] and S["has_ext"]
    check(L, S, alg, kind, n, mf)
