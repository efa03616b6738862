"""Development check, CPU only: the batched COBYLA kernel (hip/cobyla_kernels.hip, one wavefront per search, lane-parallel) compiled by
g++ over tools/simt_emu (one std::thread per lane, barriers where the kernel has them) against the product's HOST COBYLA
(cobyla_host.c over cobyla_core.h, reached through the emulated device library's nla_k_cobyla_batch: every start through
nlopt_optimize(LN_COBYLA) with the objective in the host callback's summation order).  In exact-order mode every objective value is
the host's bit for bit (sphere / Rosenbrock: no transcendental), so every decision, the evaluation count, the result code and the
minimiser must be IDENTICAL.  The GPU twin is tests/test_gpu_cobyla.py (against the real reference).
       usage: python tools/cobyla_emu_check.py [quick | tiny]"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _oracle as O          # noqa: E402

HIP = os.path.join(ROOT, "nlopt_amd", "csrc", "hip")
OUT = os.path.join(ROOT, "tools", "_build", "libcobyla_emu.so")


class Params(C.Structure):
    _fields_ = [("minf_max", C.c_double), ("ftol_rel", C.c_double), ("ftol_abs", C.c_double), ("xtol_rel", C.c_double),
                ("maxeval", C.c_int32), ("exact", C.c_int32), ("sign", C.c_double), ("xtol_abs", C.c_void_p), ("abort", C.c_void_p), ("done", C.c_void_p)]


class Result(C.Structure):
    _fields_ = [("f", C.c_double), ("ret", C.c_int32), ("nevals", C.c_int32), ("iterm", C.c_int32), ("cols", C.c_int32)]


OUT_GLOBAL = os.path.join(ROOT, "tools", "_build", "libcobyla_global_emu.so")


def build(src="cobyla_kernels.hip", out=OUT):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    srcs = [os.path.join(HIP, src)]
    deps = srcs + [os.path.join(HIP, "cobyla_search.h"), os.path.join(HIP, "local_common.h"), os.path.join(HIP, "dev_common.h")]
    if os.path.exists(out) and all(os.path.getmtime(out) > os.path.getmtime(s) for s in deps):
        return out
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-x", "c++", "-w", "-I", os.path.join(ROOT, "tools", "simt_emu"),
                    "-o", out] + srcs + ["-lpthread"], check=True)
    return out


def build_global():
    """hip/cobyla_global.hip (the same search, its matrices in a global-memory workspace) the same way: tests/test_cobyla_global_emu.py"""
    return build("cobyla_global.hip", OUT_GLOBAL)


def run(L, obj, n, starts, lo, hi, xtol_rel=1e-6, maxeval=0, ftol_rel=0.0, dx=None, exact=1, sign=1.0, minf_max=-np.inf, entry="nla_k_cobyla_batch"):
    count, ld = starts.shape[0], (n + 1) & ~1
    X = np.zeros((count, ld)); X[:, :n] = starts
    lb = np.ascontiguousarray(lo, dtype=np.float64); ub = np.ascontiguousarray(hi, dtype=np.float64)
    nwork = max(8, count * 8)
    if entry == "nla_k_cobyla_batch_global":
        L.nla_cobyla_global_work_doubles.restype = C.c_size_t
        nwork = L.nla_cobyla_global_work_doubles(n, count)
    work = np.full(nwork, np.nan if entry == "nla_k_cobyla_batch_global" else 0.0); iwork = np.zeros(max(8, count * 8), dtype=np.int32)        # (the global kernel zeroes what it uses itself)
    res = (Result * count)()
    P = Params(minf_max, ftol_rel, 0.0, xtol_rel, maxeval, exact, sign, None, None, None)
    vp = C.c_void_p
    fn = getattr(L, entry)
    fn.argtypes = [C.c_int] * 4 + [vp] * 6 + [C.POINTER(Params), vp, vp]
    fn.restype = C.c_int
    rc = fn(O.OBJ[obj], n, ld, count, lb.ctypes.data, ub.ctypes.data, dx.ctypes.data if dx is not None else None, X.ctypes.data,
            work.ctypes.data, iwork.ctypes.data, C.byref(P), C.cast(res, vp), None)
    assert rc == 0, rc
    return dict(x=X[:, :n].copy(), f=np.array([r.f for r in res]), ret=[r.ret for r in res], nevals=[r.nevals for r in res])


OUT_EXT = os.path.join(ROOT, "tools", "_build", "libcobyla_ext_emu.so")


def build_ext():
    """hip/cobyla_ext.hip (the same search as a coroutine around an objective outside the kernel) the same way: tests/test_cobyla_ext_emu.py"""
    return build("cobyla_ext.hip", OUT_EXT)


class Ext(C.Structure):
    """nla_local_ext (include/nlopt_amd.h)"""
    _fields_ = [("req", C.c_void_p), ("EX", C.c_void_p), ("EG", C.c_void_p), ("EF", C.c_void_p), ("save", C.c_void_p),
                ("resume", C.c_int32), ("forced", C.c_int32), ("timeout", C.c_int32), ("pad", C.c_int32)]


class HostMem:
    """the buffers of run_ext in host memory (the emulated kernel); tests/test_gpu_cobyla_ext.py has the device's"""
    class Buf:
        def __init__(self, a):
            self.a = a; self.ptr = a.ctypes.data

    def alloc(self, nbytes, fill=0):
        return self.Buf(np.full(max(int(nbytes), 8), fill, dtype=np.uint8))

    def put(self, a):
        return self.Buf(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy())

    def write(self, buf, a):
        buf.a[:a.nbytes] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)

    def read(self, buf, dtype, count):
        return buf.a[:np.dtype(dtype).itemsize * count].view(dtype).copy()

    def sync(self):
        pass


def ext_bind(L):
    vp = C.c_void_p
    L.nla_cobyla_ext_work_doubles.restype = C.c_size_t; L.nla_cobyla_ext_work_doubles.argtypes = [C.c_int, C.c_int]
    L.nla_cobyla_save_bytes.restype = C.c_size_t; L.nla_cobyla_save_bytes.argtypes = [C.c_int]
    L.nla_k_cobyla_batch_ext.restype = C.c_int
    L.nla_k_cobyla_batch_ext.argtypes = [C.c_int] * 3 + [vp] * 5 + [C.POINTER(Params), vp, C.POINTER(Ext), vp]
    return L


def run_ext(L, n, starts, lo, hi, evaluate, xtol_rel=1e-6, maxeval=0, ftol_rel=0.0, dx=None, minf_max=-np.inf, forced_from=None, mem=None,
            max_steps=1000000):
    """the host side of the coroutine nla_k_cobyla_batch_ext: launch, read req, evaluate every waiting row of EX with `evaluate`
    (the value goes into EF as it comes: the caller applies a maximisation's sign), launch again with resume = 1 until no search
    waits.  forced_from = k: ext.forced = 1 from the k-th relaunch on (the first launch is number 0).  `asked`: per search, the
    points it requested in order; `finished_at`: the launch after which its state was 2; `seen`: states after every launch."""
    ext_bind(L)
    mem = mem or HostMem()
    count, ld = starts.shape[0], (n + 1) & ~1
    X = np.zeros((count, ld)); X[:, :n] = starts
    bX, bl, bu = mem.put(X), mem.put(np.asarray(lo, dtype=np.float64)), mem.put(np.asarray(hi, dtype=np.float64))
    bd = mem.put(np.asarray(dx, dtype=np.float64)) if dx is not None else None
    # NaN everywhere a starting search must not rely on: it zeroes its slice itself and writes its record before it reads it
    bw = mem.alloc(8 * L.nla_cobyla_ext_work_doubles(n, count), 0xff)
    bsave, breq = mem.alloc(L.nla_cobyla_save_bytes(n) * count, 0xff), mem.put(np.zeros((count, 2), dtype=np.int32))
    bEX, bEG, bEF = mem.put(np.full((count, ld), np.nan)), mem.put(np.full(8, np.nan)), mem.put(np.full(count, np.nan))
    bo = mem.alloc(C.sizeof(Result) * count)
    P = Params(minf_max, ftol_rel, 0.0, xtol_rel, maxeval, 0, 1.0, None, None, None)
    E = Ext(breq.ptr, bEX.ptr, bEG.ptr, bEF.ptr, bsave.ptr, 0, 0, 0, 0)
    asked, finished_at, seen, step = [[] for _ in range(count)], [None] * count, [], 0
    while True:
        E.forced = 1 if forced_from is not None and step >= forced_from else 0
        rc = L.nla_k_cobyla_batch_ext(n, ld, count, bl.ptr, bu.ptr, bd.ptr if bd else None, bX.ptr, bw.ptr, C.byref(P), bo.ptr, C.byref(E), None)
        assert rc == 0, rc
        mem.sync()
        state = mem.read(breq, np.int32, 2 * count).reshape(count, 2)[:, 0]
        seen.append(state.copy())
        for i in range(count):
            if state[i] == 2 and finished_at[i] is None:
                finished_at[i] = step
        waiting = [i for i in range(count) if state[i] == 1]
        if not waiting:
            break
        assert step < max_steps
        EX, EF = mem.read(bEX, np.float64, count * ld).reshape(count, ld), mem.read(bEF, np.float64, count)
        for i in waiting:
            asked[i].append(EX[i, :n].copy())
            EF[i] = evaluate(EX[i, :n].copy())
        mem.write(bEF, EF)
        E.resume = 1
        step += 1
    res = (Result * count).from_buffer_copy(mem.read(bo, np.uint8, C.sizeof(Result) * count).tobytes())
    return dict(x=mem.read(bX, np.float64, count * ld).reshape(count, ld)[:, :n].copy(), f=np.array([r.f for r in res]), ret=[r.ret for r in res],
                nevals=[r.nevals for r in res], asked=asked, finished_at=finished_at, seen=seen, launches=step + 1)


OUT_CON = os.path.join(ROOT, "tools", "_build", "libcobyla_con_emu.so")


def build_con():
    """hip/cobyla_con.hip (the coroutine with the caller's nonlinear constraint values as rows in front of the bound rows) the same
    way: tests/test_cobyla_con_emu.py"""
    return build("cobyla_con.hip", OUT_CON)


def con_bind(L):
    vp = C.c_void_p
    L.nla_cobyla_con_serves.restype = C.c_int; L.nla_cobyla_con_serves.argtypes = [C.c_int, C.c_int]
    L.nla_cobyla_con_work_doubles.restype = C.c_size_t; L.nla_cobyla_con_work_doubles.argtypes = [C.c_int] * 3
    L.nla_cobyla_con_save_bytes.restype = C.c_size_t; L.nla_cobyla_con_save_bytes.argtypes = [C.c_int, C.c_int]
    L.nla_k_cobyla_batch_ext_con.restype = C.c_int
    L.nla_k_cobyla_batch_ext_con.argtypes = [C.c_int] * 3 + [vp] * 5 + [C.POINTER(Params), vp, C.POINTER(Ext)] + [C.c_int] * 3 + [vp] * 4
    return L


def con_rowmap(mi, eq_sizes):
    """row -> column of EC (c >= 0: +EC[c], c < 0: -EC[-c - 1]) in the reference's order (cobyla.c:106-119): the mi inequality rows
    negated, then per equality BLOCK its values followed by the same block's values negated"""
    rows, c0 = [-(k + 1) for k in range(mi)], mi
    for b in eq_sizes:
        rows += [c0 + j for j in range(b)] + [-(c0 + j + 1) for j in range(b)]
        c0 += b
    return np.array(rows, dtype=np.int32)


def run_ext_con(L, n, starts, lo, hi, evaluate, mi, eq_sizes, tol=None, xtol_rel=1e-6, maxeval=0, ftol_rel=0.0, dx=None, minf_max=-np.inf,
                forced_from=None, mem=None, max_steps=1000000):
    """run_ext for nla_k_cobyla_batch_ext_con: evaluate(x) returns (f, the mi inequality values, the equality values block after
    block); f goes into EF as it comes, the values into the search's row of EC.  eq_sizes: the sizes of the equality blocks; tol: mi +
    me tolerances by column (None: zeros).  EC starts as NaN and only the rows of WAITING searches are ever written: a search that
    read a row it did not ask for would go wrong.  Returns what run_ext returns."""
    con_bind(L)
    mem = mem or HostMem()
    me = int(sum(eq_sizes))
    mc, ldc = mi + 2 * me, max(mi + me, 1)
    count, ld = starts.shape[0], (n + 1) & ~1
    X = np.zeros((count, ld)); X[:, :n] = starts
    bX, bl, bu = mem.put(X), mem.put(np.asarray(lo, dtype=np.float64)), mem.put(np.asarray(hi, dtype=np.float64))
    bd = mem.put(np.asarray(dx, dtype=np.float64)) if dx is not None else None
    bw = mem.alloc(8 * L.nla_cobyla_con_work_doubles(n, mc, count), 0xff)
    bsave, breq = mem.alloc(L.nla_cobyla_con_save_bytes(n, mc) * count, 0xff), mem.put(np.zeros((count, 2), dtype=np.int32))
    bEX, bEG, bEF = mem.put(np.full((count, ld), np.nan)), mem.put(np.full(8, np.nan)), mem.put(np.full(count, np.nan))
    bEC = mem.put(np.full((count, ldc), np.nan))
    btol = mem.put(np.zeros(mi + me) if tol is None else np.asarray(tol, dtype=np.float64))
    bmap = mem.put(con_rowmap(mi, eq_sizes))
    bo = mem.alloc(C.sizeof(Result) * count)
    P = Params(minf_max, ftol_rel, 0.0, xtol_rel, maxeval, 0, 1.0, None, None, None)
    E = Ext(breq.ptr, bEX.ptr, bEG.ptr, bEF.ptr, bsave.ptr, 0, 0, 0, 0)
    asked, finished_at, seen, step = [[] for _ in range(count)], [None] * count, [], 0
    while True:
        E.forced = 1 if forced_from is not None and step >= forced_from else 0
        rc = L.nla_k_cobyla_batch_ext_con(n, ld, count, bl.ptr, bu.ptr, bd.ptr if bd else None, bX.ptr, bw.ptr, C.byref(P), bo.ptr, C.byref(E),
                                          mi, me, ldc, bEC.ptr, btol.ptr, bmap.ptr, None)
        assert rc == 0, rc
        mem.sync()
        state = mem.read(breq, np.int32, 2 * count).reshape(count, 2)[:, 0]
        seen.append(state.copy())
        for i in range(count):
            if state[i] == 2 and finished_at[i] is None:
                finished_at[i] = step
        waiting = [i for i in range(count) if state[i] == 1]
        if not waiting:
            break
        assert step < max_steps
        EX, EF = mem.read(bEX, np.float64, count * ld).reshape(count, ld), mem.read(bEF, np.float64, count)
        EC = mem.read(bEC, np.float64, count * ldc).reshape(count, ldc)
        for i in waiting:
            asked[i].append(EX[i, :n].copy())
            f, g, h = evaluate(EX[i, :n].copy())
            EF[i] = f
            EC[i, :mi + me] = np.concatenate([np.asarray(g, dtype=np.float64).reshape(-1), np.asarray(h, dtype=np.float64).reshape(-1)])
        mem.write(bEF, EF); mem.write(bEC, EC)
        E.resume = 1
        step += 1
    res = (Result * count).from_buffer_copy(mem.read(bo, np.uint8, C.sizeof(Result) * count).tobytes())
    return dict(x=mem.read(bX, np.float64, count * ld).reshape(count, ld)[:, :n].copy(), f=np.array([r.f for r in res]), ret=[r.ret for r in res],
                nevals=[r.nevals for r in res], asked=asked, finished_at=finished_at, seen=seen, launches=step + 1)


def main():
    quick =len(sys.argv) > 1 and sys.argv[1] == "quick"
    build()
    K = C.CDLL(OUT)                                                        # the kernel on 64 lockstep CPU threads
    H = C.CDLL(os.path.join(ROOT, "oracle", "libnlopt_amd_emu.so"))        # the host algorithm
    rng = np.random.default_rng(11)
    #        obj, n, count, maxeval, xtol_rel, kind of box
    cases = [("sphere", 2, 3, 0, 1e-6, "plain"), ("rosenbrock", 3, 3, 0, 1e-6, "plain"), ("rosenbrock", 6, 2, 600, 1e-7, "plain"),
             ("sphere", 5, 3, 0, 1e-6, "onbound"), ("rosenbrock", 4, 2, 0, 1e-5, "halfinf"), ("sphere", 7, 2, 0, 1e-6, "steps"),
             ("rosenbrock", 12, 2, 1500, 1e-6, "plain"), ("sphere", 24, 1, 0, 1e-4, "plain"), ("rosenbrock", 33, 1, 1200, 1e-4, "onbound")]
    if quick:
        cases = cases[:4]
    if len(sys.argv) > 1 and sys.argv[1] == "tiny":           # seconds: tests/test_host_logic.py runs this
        cases = [("sphere", 2, 2, 0, 1e-6, "plain"), ("sphere", 5, 2, 0, 1e-6, "onbound"), ("rosenbrock", 6, 1, 300, 1e-7, "plain"), ("rosenbrock", 4, 1, 400, 1e-5, "halfinf"),
                 ("sphere", 7, 1, 0, 1e-5, "steps")]
    bad = 0
    for obj, n, count, maxeval, xtol, kind in cases:
        _, lo, hi = O.golden_x0(obj, n)
        lov, hiv = np.full(n, float(lo)), np.full(n, float(hi))
        starts = rng.uniform(lo, hi, (count, n))
        dx = None
        if kind == "onbound":
            starts[0, : max(1, n // 3)] = hi
            starts[-1, -1] = lo
        if kind == "halfinf":
            hiv[0] = np.inf; lov[1] = -np.inf
            if n > 2:
                lov[2] = -np.inf; hiv[2] = np.inf
        if kind == "steps":
            dx = np.linspace(0.3, 1.7, n) * 0.1 * (hi - lo)
        a = run(K, obj, n, starts, lov, hiv, xtol_rel=xtol, maxeval=maxeval, dx=dx)
        b = run(H, obj, n, starts, lov, hiv, xtol_rel=xtol, maxeval=maxeval, dx=dx)
        same = a["ret"] == b["ret"] and a["nevals"] == b["nevals"] and np.array_equal(a["f"], b["f"]) and np.array_equal(a["x"], b["x"])
        print("%-10s n=%-3d %-8s kernel ret %s nevals %s f %s | host ret %s nevals %s f %s  %s"
              % (obj, n, kind, a["ret"], a["nevals"], a["f"], b["ret"], b["nevals"], b["f"], "IDENTICAL" if same else "DIFFERENT"), flush=True)
        bad += 0 if same else 1
    # a fixed coordinate (lb == ub): the kernel refuses the box (include/nlopt_amd.h) — INVALID_ARGS, no evaluation, the start unchanged —
    # where the host algorithm would eliminate the coordinate as the reference does (the contract, not a comparison with the host)
    for n, fixed in ((4, [1]), (7, [0, 3, 6])):
        _, lo, hi = O.golden_x0("rosenbrock", n)
        lov, hiv = np.full(n, float(lo)), np.full(n, float(hi))
        starts = rng.uniform(lo, hi, (2, n))
        lov[fixed] = hiv[fixed] = starts[0, fixed]
        starts[:, fixed] = lov[fixed]
        a = run(K, "rosenbrock", n, starts, lov, hiv, maxeval=300)
        ok = a["ret"] == [-2, -2] and a["nevals"] == [0, 0] and np.all(a["f"] == np.inf) and np.array_equal(a["x"], starts)
        print("rosenbrock n=%-3d fixed %-9s kernel ret %s nevals %s  %s" % (n, fixed, a["ret"], a["nevals"], "REFUSED" if ok else "NOT REFUSED"), flush=True)
        bad += 0 if ok else 1
    print("cobyla emu check:", "ok" if bad == 0 else "%d case(s) differ" % bad)
    return bad


if __name__ == "__main__":
    sys.exit(main())
