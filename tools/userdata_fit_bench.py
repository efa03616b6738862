"""What a device objective that reads data buys a least-squares fit (include/nlopt_amd_device.h: NLOPT_AMD_DEVICE_RESIDUALS).

Problem: NLOPT_GN_CRS2_LM fits y = a exp(-b t) + c (n = 3, the sample `expfit` of tests/userdata/fit_models.hip) to m data points,
population 100 000, a fixed budget of evaluations, the same seed, run two ways:
  device   the residual kernel bound with nlopt_amd_set_min_device_objective, the data handed over with
           nlopt_amd_set_device_objective_data: one workgroup of 256 threads per candidate, populations and trial windows in one launch
  host     the same sum as an ordinary C nlopt_func (tools/userdata_fit_twin.c) through the host-callback path, one point per call on
           the caller's thread — the only way such an objective could run before
reported as candidate evaluations per second of wall time around nlopt_optimize (it ends in a device synchronise), at the flagship
m = 4096 and down a sweep of smaller m: a whole workgroup per candidate is a poor trade for a handful of residuals, and the sweep shows
whether the host path overtakes it.  One device run of this budget lasts about a tenth of a second, so the device figure is the total over
DEVICE_REPS identical runs (slowest and fastest run beside it); m = 4096 is measured twice, alternating, to show the spread.

usage (GPU box): python tools/userdata_fit_bench.py [evaluations] [out-file]"""
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

N, POP, DEVICE_REPS = 3, 100000, 10


class FitData(C.Structure):
    _fields_ = [("m", C.c_long), ("t", C.c_void_p), ("y", C.c_void_p)]


def build(tmp):
    co, twin = os.path.join(tmp, "fit_models.hsaco"), os.path.join(tmp, "libfittwin.so")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "--genco", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "userdata", "fit_models.hip"), "-o", co], check=True)
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", os.path.join(ROOT, "tools", "userdata_fit_twin.c"), "-o", twin, "-lm"], check=True)
    return co, C.CDLL(twin)


def problem(m):
    t = np.linspace(0.0, 4.0, m)
    return t, 2.5 * np.exp(-1.3 * t) + 0.5 + 0.01 * np.sin(29.0 * np.arange(m))


def run(L, co, twin, device, m, evals):
    t, y = problem(m)
    o = nlopt_amd.Opt(nlopt_amd.GN_CRS2_LM, N)
    o.set_lower_bounds([0.1, 0.1, -1.0])
    o.set_upper_bounds([5.0, 5.0, 2.0])
    if device:
        assert o.set_min_device_objective(co, "expfit") > 0, o.get_errmsg()
        assert o.set_device_objective_data(np.concatenate([t, y])) > 0, o.get_errmsg()
    else:
        fd = FitData(m, t.ctypes.data, y.ctypes.data)
        o._keep += [fd, t, y]
        L.nlopt_set_min_objective.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        assert L.nlopt_set_min_objective(o._h, C.cast(twin.expfit_twin, C.c_void_p), C.addressof(fd)) > 0
    o.set_population(POP)
    o.set_maxeval(evals)
    walls, nev = [], 0
    for _ in range(DEVICE_REPS if device else 1):
        nlopt_amd.srand(5)
        t0 = time.perf_counter()
        x, minf, ret = o.optimize_raw(np.array([1.0, 1.0, 0.0]))
        walls.append(time.perf_counter() - t0)
        assert ret > 0, o.get_errmsg()
        nev += o.get_numevals()
    per = nev / len(walls)
    return dict(wall=sum(walls), rate=nev / sum(walls), lo=per / max(walls), hi=per / min(walls), minf=minf, x=x, nev=nev)


def main():
    evals = int(sys.argv[1]) if len(sys.argv) > 1 else 300000
    out = sys.argv[2] if len(sys.argv) > 2 else None
    L = nlopt_amd.lib()
    lines = ["GN_CRS2_LM, expfit (tests/userdata/fit_models.hip: y = a exp(-b t) + c, n = %d), pop = %d, %d evaluations per run, seed 5; device: %d runs"
             % (N, POP, evals, DEVICE_REPS),
             "%6s  %-44s  %-24s  %7s  %s" % ("m", "device evals/s (slowest .. fastest run; total s)", "host evals/s (wall s)", "ratio", "minf device / host")]
    with tempfile.TemporaryDirectory() as tmp:
        co, twin = build(tmp)
        run(L, co, twin, True, 64, POP + 1000)                                          # warm-up: module load, allocations
        slower = []
        for m in (4096, 4096, 1024, 256, 64, 16):
            d, h = run(L, co, twin, True, m, evals), run(L, co, twin, False, m, evals)
            lines.append("%6d  %10.4g (%10.4g .. %10.4g; %6.3f)  %12.4g (%7.3f)  %6.2fx  %.12g / %.12g"
                         % (m, d["rate"], d["lo"], d["hi"], d["wall"], h["rate"], h["wall"], d["rate"] / h["rate"], d["minf"], h["minf"]))
            if d["rate"] < h["rate"]:
                slower.append(m)
    lines.append("device objective slower per evaluation than the host callback at m = %s" % (", ".join(map(str, slower)) if slower else "none of these"))
    text = "\n".join(lines)
    print(text)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
