"""What device constraint blocks buy an ISRES generation (include/nlopt_amd_device.h: NLOPT_AMD_DEVICE_CONSTRAINTS).

Problem: NLOPT_GN_ISRES, compiled-in Rastrigin, n = 256, pop = 50 000 (the shape of BASELINE.json's config 3), three inequality
constraints of tests/usercon/cons_extra.hip (g0, g1, g2).  A fixed number of generations, run twice with the same seed:
  device   the block bound with nlopt_amd_add_inequality_device_mconstraint: <name>_coneval + the fold kernel, nothing read back
  twins    the same three values as an ordinary C nlopt_mfunc (tools/isres_usercon_twin.c): the population is read back and f and the
           constraints are called on the host, point by point — the path such a problem took before
and the device time of one <name>_coneval launch at that shape (one lane per constraint walks the n coordinates: the exact choice).

usage (GPU box): python tools/isres_usercon_bench.py [generations] [out-file]"""
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nlopt_amd  # noqa: E402

N, POP, M = 256, 50000, 3


def build(tmp):
    co, twin = os.path.join(tmp, "cons_extra.hsaco"), os.path.join(tmp, "libtwin.so")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "--genco", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "usercon", "cons_extra.hip"), "-o", co], check=True)
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", os.path.join(ROOT, "tools", "isres_usercon_twin.c"), "-o", twin], check=True)
    return co, C.CDLL(twin)


def run(L, co, twin, device, gens):
    o = nlopt_amd.Opt(nlopt_amd.GN_ISRES, N)
    o.set_lower_bounds(-5.12)
    o.set_upper_bounds(5.12)
    o.set_min_objective(nlopt_amd.objective("rastrigin"))
    if device:
        assert o.add_inequality_device_constraints(co, "cons", M) > 0, o.get_errmsg()
    else:
        L.nlopt_add_inequality_mconstraint.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p]
        assert L.nlopt_add_inequality_mconstraint(o._h, M, C.cast(twin.cons_twin, C.c_void_p), None, None) > 0
    o.set_population(POP)
    o.set_maxeval(gens * POP)
    nlopt_amd.srand(5)
    t0 = time.perf_counter()
    x, minf, ret = o.optimize_raw(np.full(N, 0.25))
    wall = time.perf_counter() - t0
    st = o.stats()
    assert ret > 0, o.get_errmsg()
    return dict(wall=wall, minf=minf, x=x, nev=o.get_numevals(), st=st)


def time_coneval(L, co, reps=20):
    """device time (HIP events) of one cons_coneval launch over POP rows"""
    vp = C.c_void_p
    for nm in ("nla_module_load_file", "nla_module_function"):
        getattr(L, nm).restype = vp
    L.nla_module_load_file.argtypes = [C.c_char_p]
    L.nla_module_function.argtypes = [vp, C.c_char_p]
    L.nla_module_launch.argtypes = [vp, C.c_uint, C.c_uint, vp, vp]
    L.nla_module_unload.argtypes = [vp]
    mod = L.nla_module_load_file(co.encode())
    fn = L.nla_module_function(mod, b"cons_coneval")
    assert mod and fn
    ld, ldc = N, 4
    X = nlopt_amd.DevBuf.from_array(np.random.default_rng(1).uniform(-5.12, 5.12, size=(POP, ld)))
    Cb = nlopt_amd.DevBuf(8 * POP * ldc)
    args = [C.c_int(N), C.c_int(ld), C.c_long(POP), C.c_void_p(X.ptr), C.c_int(M), C.c_int(ldc), C.c_void_p(Cb.ptr)]
    params = (C.c_void_p * len(args))(*[C.cast(C.byref(a), C.c_void_p) for a in args])
    e0, e1 = L.nla_event_create(), L.nla_event_create()
    assert L.nla_module_launch(fn, (POP + 3) // 4, 256, params, None) == 0 and L.nla_stream_sync(None) == 0      # warm-up
    L.nla_event_record(e0, None)
    for _ in range(reps):
        assert L.nla_module_launch(fn, (POP + 3) // 4, 256, params, None) == 0
    L.nla_event_record(e1, None)
    L.nla_event_sync(e1)
    ms = L.nla_event_elapsed_ms(e0, e1) / reps
    L.nla_event_destroy(e0); L.nla_event_destroy(e1)
    X.free(); Cb.free()
    L.nla_module_unload(mod)
    return ms


def main():
    gens = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    out = sys.argv[2] if len(sys.argv) > 2 else None
    L = nlopt_amd.lib()
    with tempfile.TemporaryDirectory() as tmp:
        co, twin = build(tmp)
        run(L, co, twin, True, 2)                                                      # warm-up: module loads, allocations
        runs = [(dev, run(L, co, twin, dev, gens)) for dev in (True, False, True, False)]      # alternating: the spread shows
        ms = time_coneval(L, co)
    d, h = runs[0][1], runs[1][1]
    lines = ["GN_ISRES, compiled-in Rastrigin, n = %d, pop = %d, %d inequality constraints (tests/usercon/cons_extra.hip: cons), %d generations, seed 5" % (N, POP, M, gens)]
    for name, r in ((("device blocks" if dev else "twins only (host)"), r) for dev, r in runs):
        g = max(r["nev"] // POP, 1)
        lines.append("%-18s %9.2f ms per generation   t_eval_s %.4f (%.2f ms per generation)   evals %d   minf %.15g   coneval launches %d"
                     % (name, 1e3 * r["wall"] / g, r["st"]["t_eval_s"], 1e3 * r["st"]["t_eval_s"] / g, r["nev"], r["minf"], r["st"]["isres_usercon_launches"]))
    lines.append("same result: minf relative difference %.3g, x equal: %s" % (abs(d["minf"] - h["minf"]) / max(abs(h["minf"]), 1e-300), bool(np.array_equal(d["x"], h["x"]))))
    lines.append("cons_coneval, %d rows x %d constraints, one lane per constraint: %.3f ms per launch (HIP events, mean of 20)" % (POP, M, ms))
    text = "\n".join(lines)
    print(text)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
