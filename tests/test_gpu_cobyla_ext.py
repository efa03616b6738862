"""-m gpu: the coroutine instance of the batched device COBYLA (hip/cobyla_ext.hip: the search of hip/cobyla_search.h around an objective
OUTSIDE the kernel, what GN_MLSL runs for a user-supplied device objective) on the MI355X, through libnlopt_amd.so's launcher.  The test is
the host side of the coroutine (tools/cobyla_emu_check.run_ext with device buffers): launch, read req, evaluate every waiting row of EX
with the sequential host twin of a compiled-in objective, write EF, launch again with resume = 1.  Oracle: the REAL reference's
nlopt_optimize(LN_COBYLA) on the same twin, its callback recording every point — result code, evaluation count, f, the minimiser and
the sequence of points each search asked for are the reference's bit for bit (sphere / Rosenbrock: no transcendental; the device's
+ - x / sqrt are IEEE).  What this adds to the CPU twin (tests/test_cobyla_ext_emu.py) is the device's memory model: slice, save
record, req and EX written by one launch and read by the next."""
import ctypes as C

import numpy as np
import pytest

import _oracle as O
import nlopt_amd
from test_cobyla_ext_emu import FORCED_STOP, MAXEVAL_REACHED, _tool, box, reference, same, stays_finished

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref not built")]


class DevMem:
    """run_ext's buffers in device memory"""
    def alloc(self, nbytes, fill=0):
        return nlopt_amd.DevBuf.from_array(np.full(max(int(nbytes), 8), fill, dtype=np.uint8))

    def put(self, a):
        return nlopt_amd.DevBuf.from_array(np.ascontiguousarray(a))

    def write(self, buf, a):
        L, a = nlopt_amd.lib(), np.ascontiguousarray(a)
        assert (L.nla_memcpy_h2d(buf.ptr, a.ctypes.data, a.nbytes, None) or L.nla_stream_sync(None)) == 0

    def read(self, buf, dtype, count):
        return buf.to_array(dtype, count)

    def sync(self):
        rc = nlopt_amd.lib().nla_stream_sync(None)
        assert rc == 0, nlopt_amd.lib().nla_dev_error_string(rc)


def twin(obj):
    f = nlopt_amd.NLOPT_FUNC(nlopt_amd.objective(obj))
    return lambda x: f(len(x), np.ascontiguousarray(x, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double)), None, None)


def device(n, starts, lb, ub, tw, **kw):
    return _tool().run_ext(nlopt_amd.lib(), n, starts, lb, ub, tw, mem=DevMem(), **kw)


# n = 2: the smallest simplex with a choice; n = 7, three starts that end at different times (finished searches sit through the later
# resumes); n = 6 half-infinite: fewer rows than 2n; n = 65: two trips of the lanes over a column and over the saved LDS block
@pytest.mark.parametrize("obj,n,count,maxeval,xtol,kind", [("sphere", 2, 1, 0, 1e-6, "plain"), ("rosenbrock", 7, 3, 150, 0.02, "plain"),
                                                           ("rosenbrock", 6, 1, 300, 1e-7, "halfinf"), ("rosenbrock", 65, 2, 110, 1e-6, "plain")])
def test_coroutine_cobyla_kernel_on_the_device_is_the_references_search_point_by_point(obj, n, count, maxeval, xtol, kind):
    lo, hi, lb, ub = box(obj, n, kind)
    starts = np.random.default_rng(4100 if n == 7 else 4000 + n).uniform(lo, hi, (count, n))
    tw = twin(obj)
    r = reference(obj, n, starts, lb, ub, xtol, maxeval, tw=tw)
    a = device(n, starts, lb, ub, tw, xtol_rel=xtol, maxeval=maxeval)
    same(a, r)
    stays_finished(a)
    if n == 7:
        assert len(set(r["nevals"])) == 3 and sorted(a["finished_at"]) == sorted(r["nevals"]), r["nevals"]


@pytest.mark.parametrize("k", [5, 10])
def test_forced_stop_from_the_kth_relaunch_on_the_device(k):
    """ext.forced = 1 from relaunch k on at n = 7 (k = 5 inside the initial simplex, k = n + 3 behind it): the reference whose callback
    calls nlopt_force_stop inside its k-th call"""
    n = 7
    lo, hi, lb, ub = box("rosenbrock", n)
    starts = np.random.default_rng(4500 + k).uniform(lo, hi, (2, n))
    tw = twin("rosenbrock")
    a = device(n, starts, lb, ub, tw, forced_from=k)
    same(a, reference("rosenbrock", n, starts, lb, ub, force_at=k, tw=tw))
    assert a["ret"] == [FORCED_STOP] * 2 and a["nevals"] == [k, k] and a["launches"] == k + 1


def test_more_searches_than_one_round_of_workgroups_over_the_dies():
    """130 searches of Rosenbrock n = 5 in one batch, 40 evaluations each: every search is the reference's"""
    n, count = 5, 130
    lo, hi, lb, ub = box("rosenbrock", n)
    starts = np.random.default_rng(4800).uniform(lo, hi, (count, n))
    tw = twin("rosenbrock")
    a = device(n, starts, lb, ub, tw, maxeval=40)
    same(a, reference("rosenbrock", n, starts, lb, ub, maxeval=40, tw=tw))


def test_top_of_the_served_range_just_past_the_initial_simplex():
    """n = 256 (a 3.9 MB slice, 56 KB of LDS saved and restored at every evaluation), one start, 259 evaluations"""
    n = 256
    lo, hi, lb, ub = box("rosenbrock", n)
    starts = np.random.default_rng(4900).uniform(lo, hi, (1, n))
    tw = twin("rosenbrock")
    a = device(n, starts, lb, ub, tw, maxeval=259)
    same(a, reference("rosenbrock", n, starts, lb, ub, maxeval=259, tw=tw))
    assert a["ret"] == [MAXEVAL_REACHED] and a["nevals"] == [259]
