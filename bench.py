#!/usr/bin/env python
"""bench.py — the benchmarks of BASELINE.json on MI355X.

Default workload (`--workload crs`) is the headline metric: candidate-evals/sec (+ gens-to-ftol),
NLOPT_GN_CRS2_LM, Griewank n=4096, pop=1e5 (the configuration fits one GPU: 3.3 GB of 288 GB).
A *step* is one pass of the hot path over one batch of work: `--evals-per-step` candidate evaluations of
the CRS2_LM trial loop (reflection gather-sum + objective + in-order commit, src/algs/crs/crs.c:125-156) on a
population that is already resident in HBM.  The population initialisation (crs_init) happens before the
timed region and is reported separately (`init`).  W warm-up steps, then EXACTLY K timed steps bracketed by
a barrier and a device synchronisation; value = evaluations made in the K steps / wall time, max over ranks.

Other workloads (BASELINE.json configs 3 and 4; parity for them is in tests/):
  --workload isres   NLOPT_GN_ISRES, Rastrigin n=256 + 4 block-sum inequality constraints, pop=5e4;
                     a step = one generation (pop evaluations + selection + evolution, isres.c:130-281)
  --workload mlsl    NLOPT_G_MLSL_LDS + LD_LBFGS(ftol_rel 1e-8), Ackley n=4096, 1000 samples per iteration;
                     a step = one MLSL iteration (sampling + the local searches it starts, mlsl.c:345-429)
For these the K timed steps are bracketed inside one nlopt_optimize() call by the library's generation hook
(nlopt_amd_set_progress): barrier + sync at the start of step W, again at the start of step W+K, where the
run is force-stopped.

N > 1 (launched by torchrun, one rank per GPU; SURVEY.md §8e / DESIGN.md §6):
  crs    the trial loop is one serial accept/reject chain — each rank runs an independent replica (seed+rank),
         no data-path collective, scaling = weak, value = sum over ranks
  isres  one job over all ranks (library communicator = RCCL): evaluation sharded, (f, penalty) all-gathered
         each generation; scaling = strong
  mlsl   one job over all ranks: the local searches of a batch are dealt over the ranks and the minimisers
         all-gathered; scaling = strong

Output: ONE JSON line on rank 0 with the driver's contract fields plus
  roofline     — dominant kernel of the workload: algorithmic bytes per launch / HIP-event time of the launches
                 on the stream they run on, vs 8 TB/s HBM; `traffic` = HBM bytes per launch from the committed
                 rocprofv3 PMC summaries of the same command (profiles/), corrected as MI355X_MICROARCH.md says
A plain run does only what that line needs: set-up, W warm-up steps, the K timed steps, the line.  With --full it also
measures and checks what takes runs of its own:
  cpu_baseline — the real reference NLopt (oracle/_ref, kind "reference") or the C port (kind "port") timed
                 single-threaded on this host on a bounded sample of the same workload
  gens_to_ftol — (crs) numevals/pop at NLOPT_FTOL_REACHED on the small configuration where the CPU reference can
                 reach it, with the reference's golden value beside it.
  pinned_run   — the timed run against the real reference's run of the same problem (tests/golden/)
  (crs, N = 1) other_sizes, other_workloads, nlopt_optimize_end_to_end; (crs, N > 1) config5_one_job
--dump-outputs DIR writes what the timed run hands its caller after the last step (best point x, minf, numevals) as
DIR/<name>.npy, float64; the inputs are fixed by the arguments (seed, sizes), so two builds can be compared output for output.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8 TB/s peak
STUCK = []                     # set when the one-job config-5 block of a multi-GPU run had to be abandoned (see bench_crs)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--full", action="store_true",
                    help="also the CPU baselines, the pins against the reference, gens-to-ftol, the other sizes / workloads, the end-to-end "
                         "call and (--gpus > 1) the config-5 block; a plain run times the headline alone")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps, write what the timed run returned (x, minf, numevals) as DIR/<name>.npy (float64)")
    ap.add_argument("--config5-pop", type=int, default=1000000, help="population of the one-job CRS block reported at --gpus > 1 with --full")
    ap.add_argument("--config5-n", type=int, default=4096)
    ap.add_argument("--no-config5", action="store_true")
    ap.add_argument("--config5-timeout", type=int, default=300)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", choices=("crs", "isres", "mlsl"), default="crs")
    ap.add_argument("--param", action="append", default=[], metavar="NAME=VALUE",
                    help="nlopt_set_param on the optimiser (and on MLSL's local optimiser): the library's switches, e.g. amd_forward=0, amd_isres_overlap=0")
    ap.add_argument("--exact", action="store_true",
                    help="mlsl: the local optimiser sums in the reference's order (\"amd_exact_dot\" = 1: iterates bit-identical to the reference's); default: workgroup tree sums")
    ap.add_argument("--local", choices=("lbfgs", "mma"), default="lbfgs",
                    help="mlsl: lbfgs = G_MLSL_LDS with an explicit LD_LBFGS (config 4); mma = GD_MLSL_LDS with its default local optimiser LD_MMA")
    ap.add_argument("--n", type=int, default=0)
    ap.add_argument("--pop", type=int, default=0)
    ap.add_argument("--obj", default="")
    ap.add_argument("--evals-per-step", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--max-spec", type=int, default=0)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--headline-only", action="store_true", help="crs with --full: skip the other sizes / workloads / end-to-end call (tuning runs)")
    ap.add_argument("--cpu-sample-pop", type=int, default=0)
    ap.add_argument("--cpu-sample-trials", type=int, default=400)
    ap.add_argument("--detail", default="", metavar="PATH",
                    help="where the FULL record goes (host_split, phases, sample strings, latency models ...); not written without it. "
                         "The printed line is the compact form of it (kept below the 8 KB of stdout a driver record keeps)")
    ap.add_argument("--full-line", action="store_true", help="print the full record as the JSON line (what rounds 1-4 printed)")
    a = ap.parse_args()
    dflt = {"crs": (4096, 100000, "griewank"), "isres": (256, 50000, "rastrigin"), "mlsl": (4096, 1000, "ackley")}[a.workload]
    a.n = a.n or dflt[0]
    a.pop = a.pop or dflt[1]
    a.obj = a.obj or dflt[2]
    return a


# ------------------------------------------------------------------------------------------------
# CPU baselines: the real reference (oracle/_ref) on a bounded sample of the same workload
# ------------------------------------------------------------------------------------------------
def cpu_baseline_crs(obj, n, pop_sample, trials, seed):
    """single-thread CPU reference on a bounded sample: init (untimed) + `trials` trial-phase
    evaluations of the same workload at the same n (the trial-phase rate does not depend on pop:
    SURVEY.md §6, 49.9 vs 50.3 evals/s at pop 2e4 vs 1e5)."""
    import _oracle as O

    class Timer(C.Structure):
        _fields_ = [("inner", C.c_void_p), ("inner_data", C.c_void_p), ("mark", C.c_long), ("count", C.c_long),
                    ("t_first", C.c_double), ("t_mark", C.c_double), ("t_last", C.c_double)]

    P = O.port()
    xs, lo, hi = O.golden_x0(obj, n)
    x = np.array(xs)
    lb, ub = np.full(n, lo), np.full(n, hi)
    tm = Timer(P.orc_objective(O.OBJ[obj]), None, pop_sample, 0, 0.0, 0.0, 0.0)
    cb = C.cast(P.orc_timing_callback, C.c_void_p).value
    me = pop_sample + trials
    minf = C.c_double()
    if O.have_ref():
        R = O.ref()
        opt = R.nlopt_create(19, n)
        R.nlopt_set_lower_bounds(opt, O.dptr(lb))
        R.nlopt_set_upper_bounds(opt, O.dptr(ub))
        R.nlopt_set_min_objective(opt, cb, C.cast(C.pointer(tm), C.c_void_p))
        R.nlopt_set_population(opt, pop_sample)
        R.nlopt_set_maxeval(opt, me)
        R.nlopt_srand(seed)
        R.nlopt_optimize(opt, O.dptr(x), C.byref(minf))
        R.nlopt_destroy(opt)
        kind = "reference"
    else:
        st = O.OrcStop()
        P.orc_stop_default(C.byref(st), n)
        st.maxeval = me
        P.orc_srand(seed)
        P.orc_crs_minimize(n, cb, C.cast(C.pointer(tm), C.c_void_p), O.dptr(lb), O.dptr(ub), O.dptr(x), C.byref(minf),
                           C.byref(st), pop_sample, None)
        kind = "port"
    ntrial = tm.count - tm.mark
    dt = tm.t_last - tm.t_mark
    return dict(value=ntrial / dt if dt > 0 else None, unit="evals/s", cores=1, kind=kind,
                sample="NLOPT_GN_CRS2_LM %s n=%d, pop=%d init untimed (%.1f s, %.0f evals/s), then %d trial-phase evals in %.1f s, 1 thread"
                       % (obj, n, pop_sample, tm.t_mark - tm.t_first, tm.mark / max(tm.t_mark - tm.t_first, 1e-9), ntrial, dt),
                init_evals_per_s=tm.mark / max(tm.t_mark - tm.t_first, 1e-9))


def cpu_baseline_isres(obj, n, pop_sample, seed, ncon=4):
    """ISRES on the CPU is dominated by the O(pop^2) stochastic ranking (isres.c:207-228): evals/s falls ~1/pop, so a smaller
    population says little.  The sample is ONE whole generation (evaluate, rank, evolve) of the real reference at the population
    it is given — at the benchmark's pop = 5e4 that is ~85-110 s on one core — timed in this run on this host: maxeval = pop + 1
    ends the run at the second evaluation of generation 2."""
    import _oracle as O
    t0 = time.perf_counter()
    if O.have_ref():
        r = O.run_ref_isres(obj, n, pop_sample, seed, nineq=ncon, maxeval=pop_sample + 1, record=False)
        kind = "reference"
    else:
        r = O.run_port_isres(obj, n, pop_sample, seed, nineq=ncon, maxeval=pop_sample + 1, record=False)
        kind = "port"
    dt = time.perf_counter() - t0
    return dict(value=pop_sample / dt, unit="evals/s", cores=1, kind=kind,
                sample="NLOPT_GN_ISRES %s n=%d + %d inequality constraints at pop=%d: one whole generation (%d evaluations, the stochastic ranking, "
                       "the mutation) in %.1f s, 1 thread" % (obj, n, ncon, pop_sample, pop_sample, dt),
                sample_pop=pop_sample, seconds_per_generation=dt)


def cpu_baseline_mlsl(obj, n, nsamples, seed, maxeval, local="lbfgs"):
    import _oracle as O
    t0 = time.perf_counter()
    if O.have_ref():
        if local == "mma":
            r = O.run_ref_mlsl(obj, n, nsamples, seed, alg=23, local=None, ftol_rel=1e-8, maxeval=maxeval, record=False)
        else:
            r = O.run_ref_mlsl(obj, n, nsamples, seed, alg=39, maxeval=maxeval, record=False)
        kind = "reference"
    else:
        r = O.run_port_mlsl(obj, n, nsamples, seed, maxeval=maxeval, record=False, local=local, lds=(n <= 1111))
        kind = "port"
    dt = time.perf_counter() - t0
    return dict(value=r["nevals"] / dt, unit="evals/s", cores=1, kind=kind,
                sample="%s %s n=%d, %d samples/iteration, the first %d evaluations of the same run in %.1f s, 1 thread"
                       % ("NLOPT_GD_MLSL_LDS (default local optimiser LD_MMA, ftol_rel 1e-8)" if local == "mma" else
                          "NLOPT_G_MLSL_LDS + LD_LBFGS(ftol_rel 1e-8)", obj, n, nsamples, r["nevals"], dt))


def gens_to_ftol():
    """gens-to-ftol on the configurations where the reference can reach it (BASELINE.md's two pins, committed as
    golden vectors from the real reference): CRS2_LM Rastrigin seed 42, n=10 pop=100 ftol_rel=1e-4 -> 5385 evals = 53.85
    'generations'; n=64 pop=2000 ftol_rel=1e-6 -> 191387 evals = 95.69 generations (minf 7.9706244871590783)."""
    import nlopt_amd
    import _oracle as O
    golds = json.load(open(os.path.join(ROOT, "tests", "golden", "crs_golden.json")))
    out = []
    for key, n, pop, ftol in (("rastrigin_n10_pop100_ftol1e-4", 10, 100, 1e-4), ("rastrigin_n64_pop2000_ftol1e-6", 64, 2000, 1e-6)):
        if out and "emu" in os.path.basename(nlopt_amd.LIB_PATH):      # (tests/test_bench_emulated.py: the CPU stand-in is too slow for 191 k evaluations)
            out.append(dict(config="skipped on the emulated device"))
            break
        gold = golds[key]
        xs, lo, hi = O.golden_x0("rastrigin", n)
        o = nlopt_amd.Opt(nlopt_amd.GN_CRS2_LM, n)
        o.set_lower_bounds(lo)
        o.set_upper_bounds(hi)
        o.set_min_objective(nlopt_amd.objective("rastrigin"))
        o.set_population(pop)
        o.set_ftol_rel(ftol)
        nlopt_amd.srand(42)
        t0 = time.perf_counter()
        x, minf, ret = o.optimize_raw(xs)
        dt = time.perf_counter() - t0
        out.append(dict(config="NLOPT_GN_CRS2_LM rastrigin n=%d pop=%d ftol_rel=%g seed=42" % (n, pop, ftol), result=int(ret),
                        numevals=o.get_numevals(), value=o.get_numevals() / float(pop), minf=minf, wall_s=dt,
                        reference_numevals=gold["nevals"], reference_value=gold["nevals"] / float(pop),
                        reference_minf=float.fromhex(gold["minf"]),
                        identical_to_reference=bool(o.get_numevals() == gold["nevals"] and int(ret) == gold["ret"])))
    first = dict(out[0])
    first["second_pin"] = out[1]
    return first


def pmc_traffic(kernel_prefix):
    """HBM bytes per launch of `kernel_prefix` from the newest committed rocprofv3 PMC summaries under profiles/
    (separate FETCH_SIZE / WRITE_SIZE passes of this command, values in KiB per dispatch).  Correction per
    MI355X_MICROARCH.md (HBM): FETCH_SIZE reports half of a wide coalesced read -> doubled."""
    import glob
    out = {}
    for counter, fac in (("FETCH_SIZE", 2.0), ("WRITE_SIZE", 1.0)):
        files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_%s*.csv" % counter.split("_")[0].lower())))
        for path in reversed(files):
            best = None
            for line in open(path):
                parts = line.rstrip("\n").split(",")
                if len(parts) >= 5 and parts[-4] == counter and kernel_prefix in line:
                    try:
                        cand = (float(parts[-2]), float(parts[-1]))
                    except ValueError:
                        continue
                    if best is None or cand[0] > best[0]:
                        best = cand
            if best:
                out[counter] = dict(bytes_per_launch=best[1] * 1024.0 * fac, source=os.path.relpath(path, ROOT))
                break
    if "FETCH_SIZE" not in out:
        return None, None
    total = out["FETCH_SIZE"]["bytes_per_launch"] + out.get("WRITE_SIZE", {}).get("bytes_per_launch", 0.0)
    return total, {k: v["source"] for k, v in out.items()}


# ------------------------------------------------------------------------------------------------
def main():
    a = parse()
    CRS_PARAMS[:] = list(getattr(a, "param", []) or [])
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    import torch
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if torch.cuda.is_available():
            torch.cuda.set_device(local_rank)
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
        else:                                   # tests/test_bench_emulated.py: the contract at world 2 without a GPU (emulated device layer)
            dist.init_process_group("gloo", rank=rank, world_size=world)
    import nlopt_amd
    L = nlopt_amd.lib()
    if nlopt_amd.device_count() <= 0:
        raise SystemExit("bench.py: no HIP device visible (libnlopt_amd has no CPU fallback)")
    L.nla_dev_set(local_rank)
    if torch.cuda.is_available():
        torch.cuda.set_device(local_rank)

    def sync_all():
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        L.nla_stream_sync(None)
        if dist is not None:
            dist.barrier()

    def reduce(dt, evals, sum_evals):
        if dist is None:
            return dt, float(evals)
        dev = "cuda" if torch.cuda.is_available() else "cpu"
        tt = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        te = torch.tensor([float(evals)], dtype=torch.float64, device=dev)
        dist.all_reduce(te, op=dist.ReduceOp.SUM if sum_evals else dist.ReduceOp.MAX)
        return float(tt.item()), float(te.item())

    if a.workload == "crs":
        out = bench_crs(a, nlopt_amd, L, rank, world, sync_all, reduce)
    else:
        out = bench_generational(a, nlopt_amd, L, rank, world, dist, sync_all, reduce)
    if rank == 0:
        outputs = out.pop("outputs")
        if a.dump_outputs:
            os.makedirs(a.dump_outputs, exist_ok=True)
            for name, v in outputs.items():
                np.save(os.path.join(a.dump_outputs, name + ".npy"), np.asarray(v, dtype=np.float64).reshape(-1))
        if a.detail:
            try:
                os.makedirs(os.path.dirname(os.path.abspath(a.detail)), exist_ok=True)
                with open(a.detail, "w") as fh:
                    json.dump(out, fh, indent=1)
                out["detail"] = os.path.relpath(a.detail, ROOT)
            except OSError:
                pass
        print(json.dumps(out if a.full_line else compact_line(out)), flush=True)
    if STUCK:                              # a hung collective thread is still alive: no barrier, no orderly teardown
        os._exit(0)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


# ------------------------------------------------------------------------------------------------
# the printed line: every number the contract asks for and every measured value / fraction / speed-up, none of the prose
# ------------------------------------------------------------------------------------------------
LINE_BUDGET = 7000      # bytes: a driver record keeps the last 8 KB of stdout
DROP_KEYS = ("host_split", "traffic_note", "traffic_source", "model", "peak_note", "init", "phases", "launches_timed_of_passes", "path",
             "achievable", "frac_of_achievable", "avg_algorithmic_bytes_per_launch", "evals_per_step_requested", "setup_and_teardown_s",
             "init_evals_per_s", "roofline_hbm_passes", "total_seconds_incl_setup", "reference_numevals", "reference_value", "wall_s",
             "note", "mutations", "reference_mutations", "trial_evals", "estimate_at_benchmark_pop", "sample_pop")


def _round(v):
    if isinstance(v, float):
        return float("%.6g" % v)
    return v


def _prune(v, depth=0):
    if isinstance(v, dict):
        return {k: _prune(x, depth + 1) for k, x in v.items() if k not in DROP_KEYS}
    if isinstance(v, list):
        return [_prune(x, depth + 1) for x in v]
    if isinstance(v, str) and depth > 1 and len(v) > 96:
        return v[:93] + "..."
    return _round(v)


def compact_line(full):
    """the contract's keys untouched; nested records pruned of prose and of the second-order numbers (they are in the detail file).  What
    stays per size / workload: value, ms per step, roofline (bound, kernel, achieved, peak, frac, traffic, avg launch), cpu_baseline value + kind,
    the speed-up, identical_to_reference flags"""
    out = {}
    for k, v in full.items():
        if k in ("host_split", "init"):
            continue
        if k == "config":
            out[k] = v
        elif k == "cpu_baseline":
            out[k] = {kk: (_round(x) if not isinstance(x, str) or len(x) <= 200 else x[:197] + "...") for kk, x in v.items()} if isinstance(v, dict) else v
        elif k == "roofline":
            out[k] = _prune(v, 1)
        else:
            out[k] = _prune(v, 0)
    for wl in (out.get("other_workloads") or {}).values():
        if isinstance(wl, dict):
            for kk in ("higher_is_better", "scaling", "vs_baseline", "data", "n_gpus", "metric", "final_result", "dtype"):
                wl.pop(kk, None)
    order = ["nlopt_optimize_end_to_end", "window", "gens_to_ftol"]          # what goes first if the line is still too long
    while len(json.dumps(out)) > LINE_BUDGET and order:
        k = order.pop(0)
        if k == "gens_to_ftol" and isinstance(out.get(k), dict):
            g = out[k]
            out[k] = {"value": g.get("value"), "identical_to_reference": g.get("identical_to_reference"),
                      "second_pin": {"value": (g.get("second_pin") or {}).get("value"), "identical_to_reference": (g.get("second_pin") or {}).get("identical_to_reference")}}
        elif k in out:
            out[k] = {kk: x for kk, x in out[k].items() if kk in ("value", "unit", "useful_frac", "slots_started", "slots_used")} if isinstance(out[k], dict) else out[k]
    return out


CRS_PARAMS = []        # --param NAME=VALUE of the command line (the library's A/B switches), applied to every CRS2_LM object of crs_measure


def crs_measure(nlopt_amd, L, obj, n, pop, seed, warmup, steps, evals_per_step, sync_all, max_spec=0, comm=None):
    """open a CRS2_LM run (population initialisation untimed), W warm-up steps, K timed steps; returns the raw numbers.
    comm: ONE job over the communicator's ranks (population sharded by coordinate), every rank with the same seed"""
    import _oracle as O
    xs, lo, hi = O.golden_x0(obj, n)
    o = nlopt_amd.Opt(nlopt_amd.GN_CRS2_LM, n)
    o.set_lower_bounds(lo)
    o.set_upper_bounds(hi)
    o.set_min_objective(nlopt_amd.objective(obj))
    o.set_population(pop)
    if max_spec:
        o.set_param("amd_max_spec", max_spec)
    for kv in CRS_PARAMS:
        o.set_param(kv.split("=", 1)[0], float(kv.split("=", 1)[1]))
    if comm is not None:
        o.set_comm(comm)
    nlopt_amd.srand(seed)
    x = np.array(xs)
    minf, ret = C.c_double(), C.c_int()
    if comm is not None:
        sync_all()
    t0 = time.perf_counter()
    s = L.nlopt_amd_crs_open(o._h, x.ctypes.data_as(C.POINTER(C.c_double)), C.byref(minf), C.byref(ret))
    t_init = time.perf_counter() - t0
    if not s or ret.value != 1:
        raise SystemExit("bench.py: crs_open failed: ret=%d %s" % (ret.value, o.get_errmsg()))
    for _ in range(warmup):
        if L.nlopt_amd_crs_step(s, evals_per_step) != 1:
            raise SystemExit("bench.py: the run stopped during warm-up")
    sync_all()
    st0, ev0 = o.stats(), o.get_numevals()
    t0 = time.perf_counter()
    for _ in range(steps):
        if L.nlopt_amd_crs_step(s, evals_per_step) != 1:
            raise SystemExit("bench.py: the run stopped inside the timed region")
    sync_all()
    dt = time.perf_counter() - t0
    st1, ev1 = o.stats(), o.get_numevals()
    fret = L.nlopt_amd_crs_close(s)          # writes the best point into x and minf
    return dict(dt=dt, evals=ev1 - ev0, st0=st0, st1=st1, t_init=t_init, fret=int(fret), minf=minf.value, numevals=int(ev1), x=x)


def pinned_to_reference(m, n, pop, obj, seed):
    """the run bench.py has just timed against the REAL reference's run of the same problem (tests/golden/full_crs_griewank_n4096_pop1e5_long.npz:
    N + 60 018 evaluations of oracle/_ref, written by tests/golden/make_fullsize.py): at the evaluation where this run stopped — the minimum
    found, the number of accepted trials and the number of mutation evaluations must be the reference's at that evaluation (crs.c:125-156)"""
    path = os.path.join(ROOT, "tests", "golden", "full_crs_griewank_n4096_pop1e5_long.npz")
    if (n, pop, obj, seed) != (4096, 100000, "griewank", 42) or not os.path.exists(path):
        return None
    g = np.load(path)
    k = m["numevals"] - pop
    if k < 0 or k > len(g["trial_f"]):
        return {"numevals": m["numevals"], "identical_to_reference": None, "note": "the run stopped outside the fixture's %d trial evaluations" % len(g["trial_f"])}
    ref_minf = float(g["best_f"][np.searchsorted(g["best_eval"], m["numevals"], side="right") - 1])
    ref_acc = int(g["trial_accepted"][:k].sum())
    ref_mut = int((g["trial_kind"][:k] == 2).sum())
    st = m["st1"]
    same = bool(abs(m["minf"] - ref_minf) <= 1e-10 * abs(ref_minf) and st["accepted"] == ref_acc and st["evals_mutation"] == ref_mut)
    return {"numevals": m["numevals"], "trial_evals": k, "minf": m["minf"], "reference_minf": ref_minf, "accepted": int(st["accepted"]),
            "reference_accepted": ref_acc, "mutations": int(st["evals_mutation"]), "reference_mutations": ref_mut, "identical_to_reference": same}


def pinned_isres(n, pop, obj, seed, ncon, numevals, minf, mt_words):
    """the ISRES run bench.py has just timed against the REAL reference stopped at the same evaluation (tests/golden/
    full_isres_rastrigin_n256_pop5e4_4ineq.npz `stop_*`: oracle/_ref run with maxeval = g pop + 1 — where the hook's force_stop ends this
    run, isres.c:195-198): the minimum and the position of the MT19937 stream (every ranking step, every Box-Muller attempt)"""
    path = os.path.join(ROOT, "tests", "golden", "full_isres_rastrigin_n256_pop5e4_4ineq.npz")
    if (n, pop, obj, seed, ncon) != (256, 50000, "rastrigin", 42, 4) or not os.path.exists(path):
        return None
    g = np.load(path)
    if "stop_evals" not in g.files:
        return None
    hit = np.flatnonzero(g["stop_evals"] == numevals)
    if len(hit) == 0:
        return {"numevals": int(numevals), "identical_to_reference": None, "note": "the run stopped at an evaluation the fixture has no reference stop for (%s)" % g["stop_evals"].tolist()}
    k = int(hit[0])
    ref_minf, ref_words = float(g["stop_minf"][k]), int(g["stop_words"][k])
    return {"numevals": int(numevals), "generations": k + 1, "minf": minf, "reference_minf": ref_minf, "mt_words": int(mt_words), "reference_mt_words": ref_words,
            "identical_to_reference": bool(abs(minf - ref_minf) <= 1e-10 * abs(ref_minf) and int(mt_words) == ref_words)}


def pinned_mlsl(n, pop, obj, seed, exact, iters_done, numevals, minf, trace):
    """the MLSL run bench.py has just timed against the REAL reference's run (tests/golden/full_mlsl_ackley_n4096_N1000.npz `long_*`, `stop_*`):
    every sample, which points were started from and in which order, each search's minimum and evaluation count, iteration by iteration
    (mlsl.c:349-428).  amd_exact_dot = 1 (the reference's summation order) is the PARITY mode: its evaluation counts — hence numevals and
    where maxeval would cut — are the reference's.  The default (tree-sum) mode takes the reference's decisions — same samples, same
    starts in the same order, same searches per iteration, minima to 1e-8 — with evaluation counts that drift by a few per search;
    the drift is reported."""
    path = os.path.join(ROOT, "tests", "golden", "full_mlsl_ackley_n4096_N1000.npz")
    if (n, pop, obj, seed) != (4096, 1000, "ackley", 42) or not os.path.exists(path):
        return None
    g = np.load(path)
    if "long_sloc" not in g.files or iters_done < 1 or iters_done > len(g["long_it_nloc"]):
        return None
    nloc_ref, nev_ref = int(g["long_it_nloc"][iters_done - 1]), int(g["long_it_nevals"][iters_done - 1]) + 1
    fs = trace[trace["kind"] == 3]["f"]
    fl = trace[trace["kind"] == 4]
    ns_ref = iters_done * pop
    samples_same = bool(len(fs) >= ns_ref and np.all(np.abs(fs[:ns_ref] - g["long_fsamp"][:ns_ref]) <= 1e-10 * np.maximum(np.abs(g["long_fsamp"][:ns_ref]), 1.0)))
    starts_same = bool(len(fl) == nloc_ref and np.array_equal(fl["row"], g["long_sloc"][:nloc_ref]))
    k = min(len(fl), nloc_ref)
    minima_same = bool(k > 0 and np.all(np.abs(fl["f"][:k] - g["long_floc"][:k]) <= 1e-8 * np.maximum(np.abs(g["long_floc"][:k]), 1.0)))
    drift = np.abs(fl["accepted"][:k].astype(np.int64) - g["long_eloc"][:k].astype(np.int64))
    hit = np.flatnonzero(g["stop_evals"] == nev_ref)
    ref_minf = float(g["stop_minf"][int(hit[0])]) if len(hit) else None
    minf_same = bool(ref_minf is not None and abs(minf - ref_minf) <= 1e-8 * abs(ref_minf))
    decisions = samples_same and starts_same and minima_same and minf_same
    out = {"mode": "amd_exact_dot=1 (parity mode: the reference's summation order)" if exact else "default (tree sums; decisions pinned, evaluation counts drift)",
           "iterations": int(iters_done), "numevals": int(numevals), "reference_numevals": nev_ref, "local_searches": int(len(fl)), "reference_local_searches": nloc_ref,
           "minf": minf, "reference_minf": ref_minf, "samples_identical": samples_same, "starts_identical_in_order": starts_same, "minima_within_1e-8": minima_same,
           "evaluation_count_drift": {"max": int(drift.max()) if k else None, "mean": float(drift.mean()) if k else None, "searches_identical": int((drift == 0).sum())},
           "decisions_identical_to_reference": bool(decisions),
           "identical_to_reference": bool(decisions and int(numevals) == nev_ref and (k == 0 or int(drift.max()) == 0))}
    return out


def crs_config5_one_job(a, nlopt_amd, L, rank, world, sync_all, reduce):
    """BASELINE.json config 5 (CRS2_LM Griewank n=4096, pop=1e6) as ONE job over all ranks: the population is sharded BY COORDINATE
    (every rank keeps n/world columns of every row: 32.8 GB / world), each rank runs the gather-sum, mutation and row replacement on
    its slice, the candidates of a pass are all-gathered over RCCL and every rank replays the identical chain (hip/crs_shard.hip).
    Reported: the initialisation (wall, max over ranks), the bytes all-gathered, the chain's rate."""
    import _oracle as O
    n, pop, obj = a.config5_n, a.config5_pop, "griewank"
    xs, lo, hi = O.golden_x0(obj, n)
    o = nlopt_amd.Opt(nlopt_amd.GN_CRS2_LM, n)
    o.set_lower_bounds(lo)
    o.set_upper_bounds(hi)
    o.set_min_objective(nlopt_amd.objective(obj))
    o.set_population(pop)
    comm = nlopt_amd.Comm.from_torch_distributed()
    o.set_comm(comm)
    nlopt_amd.srand(a.seed)                                   # every rank: the same stream (one job)
    x = np.array(xs)
    minf, ret = C.c_double(), C.c_int()
    sync_all()
    t0 = time.perf_counter()
    s = L.nlopt_amd_crs_open(o._h, x.ctypes.data_as(C.POINTER(C.c_double)), C.byref(minf), C.byref(ret))
    sync_all()
    t_init = time.perf_counter() - t0
    if not s or ret.value != 1:
        raise SystemExit("bench.py: config 5 crs_open failed: ret=%d %s" % (ret.value, o.get_errmsg()))
    st_i = o.stats()
    steps, per = 2, 2000
    if L.nlopt_amd_crs_step(s, per) != 1:
        raise SystemExit("bench.py: config 5 stopped during warm-up")
    sync_all()
    ev0 = o.get_numevals()
    t0 = time.perf_counter()
    for _ in range(steps):
        if L.nlopt_amd_crs_step(s, per) != 1:
            raise SystemExit("bench.py: config 5 stopped inside the timed region")
    sync_all()
    dt = time.perf_counter() - t0
    ev1 = o.get_numevals()
    minf_all = o.stats()
    L.nlopt_amd_crs_close(s)
    t_init_max, _ = reduce(t_init, 0, False)
    dt_max, evals_max = reduce(dt, ev1 - ev0, False)
    ag_ms, ag_bytes = st_i["t_allgather_ms"], st_i["allgather_bytes"]
    return {"workload": "NLOPT_GN_CRS2_LM griewank n=%d pop=%d seed=%d, ONE job over %d ranks (library communicator over RCCL)" % (n, pop, a.seed, world),
            "scaling": "strong: one job, the population sharded by coordinate over the ranks",
            "init_wall_s": t_init_max, "init_evals_per_s": pop / t_init_max,
            "allgather_ms": ag_ms, "allgather_GB_received_per_rank": ag_bytes / 1e9,
            "allgather_busbw_GBps": (ag_bytes / 1e9) * (world - 1) / world / (ag_ms / 1e3) if ag_ms > 0 else None,
            "chain_evals_per_s": evals_max / dt_max, "chain_steps": steps, "chain_evals_timed": int(evals_max),
            "population_GB_per_rank": 8.0 * n * pop / 1e9 / world, "ranks": comm.world}


def crs_end_to_end(nlopt_amd, obj, n, pop, seed, trial_evals):
    """ONE nlopt_optimize() call of the metric configuration from nlopt_create to the result: crs_init (pop evaluations) + about
    `trial_evals` trial-loop evaluations, wall clock around the call"""
    import _oracle as O
    xs, lo, hi = O.golden_x0(obj, n)
    o = nlopt_amd.Opt(nlopt_amd.GN_CRS2_LM, n)
    o.set_lower_bounds(lo)
    o.set_upper_bounds(hi)
    o.set_min_objective(nlopt_amd.objective(obj))
    o.set_population(pop)
    o.set_maxeval(pop + trial_evals)
    nlopt_amd.srand(seed)
    t0 = time.perf_counter()
    x, minf, ret = o.optimize_raw(xs)
    dt = time.perf_counter() - t0
    st = o.stats()
    ne = o.get_numevals()
    return {"call": "nlopt_optimize(NLOPT_GN_CRS2_LM %s n=%d pop=%d, maxeval=%d)" % (obj, n, pop, pop + trial_evals), "result": int(ret),
            "numevals": ne, "wall_s": dt, "evals_per_s_whole_call": ne / dt, "init_s": st["t_init_s"], "trial_s": st["t_trial_s"],
            "init_evals_per_s": st["evals_init"] / st["t_init_s"] if st["t_init_s"] > 0 else None,
            "trial_evals_per_s": (ne - st["evals_init"]) / st["t_trial_s"] if st["t_trial_s"] > 0 else None,
            "setup_and_teardown_s": dt - st["t_init_s"] - st["t_trial_s"], "minf": minf}


def bench_crs(a, nlopt_amd, L, rank, world, sync_all, reduce):
    n, pop = a.n, a.pop
    m = crs_measure(nlopt_amd, L, a.obj, n, pop, a.seed + rank, a.warmup, a.steps, a.evals_per_step, sync_all, a.max_spec)
    dt, st0, st1, t_init, fret = m["dt"], m["st0"], m["st1"], m["t_init"], m["fret"]
    dt_max, evals_all = reduce(dt, m["evals"], True)
    replicas = None
    one_job = None
    headline_one_job = None
    if world > 1:
        # N GPUs: the metric configuration as ONE job over all ranks — the population sharded by coordinate, the candidates of a pass
        # all-gathered over RCCL (hip/crs_shard.hip) — is the headline (strong scaling).  The replica figure measured above stays in
        # the line as the fallback: the one-job run goes under a watchdog, because a communicator that never comes up (RCCL's
        # bootstrap did not return on one box in round 1) or a hung collective must not take the whole line with it
        import threading
        replicas = {"value": evals_all / dt_max, "unit": "evals/s", "what": "sum over %d independent replicas (seed+rank), no collective" % world,
                    "ms_per_step": 1e3 * dt_max / a.steps}
        box1 = {}

        def job1():
            try:
                lr = int(os.environ.get("LOCAL_RANK", "0"))      # the current HIP device is a per-thread setting
                L.nla_dev_set(lr)
                try:
                    import torch
                    if torch.cuda.is_available():
                        torch.cuda.set_device(lr)
                except ImportError:
                    pass
                comm = nlopt_amd.Comm.from_torch_distributed()
                mm = crs_measure(nlopt_amd, L, a.obj, n, pop, a.seed, a.warmup, a.steps, a.evals_per_step, sync_all, a.max_spec, comm=comm)
                dtm, evm = reduce(mm["dt"], mm["evals"], False)
                tim, _ = reduce(mm["t_init"], 0, False)
                box1["r"] = dict(m=mm, dt=dtm, evals=evm, t_init=tim, ranks=comm.world, transport="rccl" if os.environ.get("NLA_BENCH_TRANSPORT", "") != "host" else "host")
            except (Exception, SystemExit) as e:
                box1["r"] = {"error": repr(e)}
        th1 = threading.Thread(target=job1, daemon=True)
        th1.start()
        th1.join(a.config5_timeout)
        if th1.is_alive():
            headline_one_job = {"error": "did not finish within %d s (communicator bootstrap or a collective hung)" % a.config5_timeout}
            STUCK.append(True)
        else:
            headline_one_job = box1.get("r")
        if headline_one_job and "error" not in headline_one_job:
            m = headline_one_job["m"]
            dt, st0, st1, t_init, fret = m["dt"], m["st0"], m["st1"], headline_one_job["t_init"], m["fret"]
            dt_max, evals_all = headline_one_job["dt"], headline_one_job["evals"]
    sharded = bool(world > 1 and headline_one_job and "error" not in headline_one_job)
    if world > 1 and a.full and not a.no_config5 and not STUCK:
        # BASELINE.json config 5 is the only CRS configuration with multi-GPU work in it: ONE job over all ranks.
        # It runs under a watchdog: the replica value above is already measured, and a communicator that never comes up (RCCL's
        # bootstrap did not return on one box in round 1) must not take the whole line with it
        import threading
        box = {}

        def job():
            try:
                lr = int(os.environ.get("LOCAL_RANK", "0"))      # the current HIP device is a per-thread setting
                L.nla_dev_set(lr)
                try:
                    import torch
                    if torch.cuda.is_available():
                        torch.cuda.set_device(lr)
                except ImportError:
                    pass
                box["r"] = crs_config5_one_job(a, nlopt_amd, L, rank, world, sync_all, reduce)
            except (Exception, SystemExit) as e:
                box["r"] = {"error": repr(e)}
        th = threading.Thread(target=job, daemon=True)
        th.start()
        th.join(a.config5_timeout)
        if th.is_alive():
            one_job = {"error": "did not finish within %d s (communicator bootstrap or a collective hung); the replica value is unaffected" % a.config5_timeout}
            STUCK.append(True)            # main() prints the line and leaves without the closing barrier
        else:
            one_job = box.get("r")
    if rank != 0:
        return None
    g_ms = st1["t_gather_ms"] - st0["t_gather_ms"]
    g_bytes = (st1["gather_bytes"] - st0["gather_bytes"]) / (world if sharded else 1)      # a rank of a sharded job moves 1/world of every row
    g_launch = st1["gather_launches"] - st0["gather_launches"]
    achieved = (g_bytes / 1e9) / (g_ms / 1e3) if g_ms > 0 else None
    slots = st1["slots_launched"] - st0["slots_launched"]
    used = st1["slots_used"] - st0["slots_used"]
    # below n = 2048 the engine times a SAMPLE of the launches (one pass in 8, one window in 4): bytes and time are of the same launches,
    # the consumed trials are of all passes — scaled to the sample
    passes = st1["rounds"] - st0["rounds"]
    timed_share = (g_launch / passes) if passes else 1.0
    useful_gbs = (used * timed_share * 8.0 * n * (n + 1) / (world if sharded else 1) / 1e9) / (g_ms / 1e3) if g_ms > 0 else None
    # the gather kernel of this run: device-resolved windows (hip/crs_chain.hip) at every dimension; the conservative passes with
    # --param amd_forward=0 and, on column slices, in a sharded job
    fw = [kv.split("=", 1)[1] for kv in CRS_PARAMS if kv.split("=", 1)[0] == "amd_forward"]         # (--param amd_forward=0/1: the A/B switch)
    # a sharded job runs device-resolved windows too since round 6 (the slices cross between the ranks' kernels through peer-mapped memory);
    # it falls back to conservative passes + one all-gather per pass where that cannot be set up: told apart by the slots a pass starts
    sh_windows = sharded and passes > 0 and slots / passes > 32
    chain = (float(fw[-1]) != 0 if fw else True) and (not sharded or sh_windows)
    gkernel = "crs_chain_kernel" if chain else "crs_advance_kernel"
    traffic, traffic_src = pmc_traffic(gkernel) if (n, pop, a.obj) == (4096, 100000, "griewank") else (None, None)
    out = {
        "metric": "candidate-evals/sec, CRS2_LM n=%d pop=%d (trial phase)" % (n, pop),
        "value": evals_all / dt_max, "unit": "evals/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
        "ms_per_step": 1e3 * dt_max / a.steps, "higher_is_better": True, "scaling": "strong" if sharded else "weak", "vs_baseline": None,
        "dtype": "f64", "data": "synthetic",
        "config": {"workload": "NLOPT_GN_CRS2_LM %s n=%d pop=%d seed=%d, %d candidate evals per step, population resident in HBM%s"
                               % (a.obj, n, pop, a.seed, a.evals_per_step,
                                  "" if world == 1 else ("; ONE job over %d ranks: population sharded by coordinate (%d columns per rank), %s (communicator ranks: %d)"
                                                         % (world, (n + world - 1) // world,
                                                            "windows resolved on every device, each rank's columns of every trial point stored into all ranks' buffers inside the launch (peer-mapped memory over xGMI, no collective per window)"
                                                            if sh_windows else "candidates of a pass all-gathered over RCCL", headline_one_job["ranks"])
                                                         if sharded else "; %d independent replicas (seed+rank)" % world)),
                   "evals_timed": int(evals_all), "evals_per_step_requested": a.evals_per_step},
        "roofline": {"bound": "hbm", "kernel": gkernel, "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": (achieved / HBM_PEAK_GBS) if achieved else None,
                     # `achieved` counts the bytes of every slot a launch STARTED (all of them are gathered in full); what the chain then
                     # CONSUMED (a slot behind a rejected one is a mutation block, a new best point restarts the window) is less:
                     "achieved_useful": useful_gbs, "frac_useful": (useful_gbs / HBM_PEAK_GBS) if useful_gbs else None,
                     # the guide's figure for what the part sustains on a streaming read (MI355X_MICROARCH.md: "8 TB/s peak (spec);
                     # ~6.3 TB/s achievable"); `frac` above stays against the spec peak
                     "achievable": 6300.0, "frac_of_achievable": (achieved / 6300.0) if achieved else None,
                     "traffic": traffic, "traffic_source": traffic_src,
                     "traffic_note": ("NOT measured in this run: HBM bytes per launch read from the committed rocprofv3 PMC passes of the same "
                                      "command (profiles/, FETCH_SIZE doubled per MI355X_MICROARCH.md + WRITE_SIZE)") if traffic else None,
                     "launches": int(g_launch), "avg_launch_ms": (g_ms / g_launch) if g_launch else None,
                     "algorithmic_bytes_per_trial": 8 * n * (n + 1),
                     "avg_algorithmic_bytes_per_launch": (g_bytes / g_launch) if g_launch else None,
                     "avg_trials_consumed_per_launch": (used * timed_share / g_launch) if g_launch else None,
                     "launches_timed_of_passes": [int(g_launch), int(passes)]},
        "window": {"slots_started": int(slots), "slots_used": int(used), "slots_recomputed_or_dropped": int(st1["slots_invalid"] - st0["slots_invalid"]),
                   "useful_frac": (used / slots) if slots else None,
                   "newbest": int(st1["slots_newbest"] - st0["slots_newbest"]),
                   "role": int(st1["slots_role"] - st0["slots_role"]),
                   "accepted": int(st1["accepted"] - st0["accepted"])},
        # where the trial phase's wall time goes on the host's side (seconds over the timed steps): inside the engine call (launches, waiting
        # for the device, copies out of pinned memory), in the in-order walk over the finished slots, the rest = preparing the pass
        "host_split": {"trial_s": st1["t_trial_s"] - st0["t_trial_s"], "engine_s": st1["t_engine_s"] - st0["t_engine_s"],
                       "walk_s": st1["t_walk_s"] - st0["t_walk_s"], "gather_kernel_s": g_ms / 1e3, "passes": int(st1["rounds"] - st0["rounds"]),
                       # the driver's ordered set: redraws of its list of worst rows, how many of them ran beside the device, their time
                       "list_refreshes": int(st1["list_refreshes"] - st0["list_refreshes"]),
                       "list_refreshes_beside_device": int(st1["list_refreshes_beside_device"] - st0["list_refreshes_beside_device"]),
                       "list_refresh_s": st1["t_list_refresh_s"] - st0["t_list_refresh_s"]},
        "init": {"evals": pop, "seconds": t_init, "init_evals_per_s": pop / t_init},
        "final_result": int(fret), "minf": m["minf"],
        "outputs": {"x": m["x"], "minf": m["minf"], "numevals": m["numevals"]},
    }
    if a.full and (world == 1 or sharded):
        pin = pinned_to_reference(m, n, pop, a.obj, a.seed)
        if pin:
            out["pinned_run"] = pin
    if a.full and world == 1 and (n, pop, a.obj) == (4096, 100000, "griewank") and not a.headline_only:
        # north_star asks for n in {64, 512, 4096}: the two smaller sizes (512 = BASELINE config 2), shorter runs, same contract
        out["other_sizes"] = {}
        for n2 in (512, 64):
            try:
                # ten steps that together consume ONE batch of pre-digested stream blocks (2^28 words / 2n blocks: crs_engine.c): the generator
                # and the Vitter kernel prepare the next batch in the background while a batch is consumed, and a sample much shorter than
                # a batch has all of that background work inside it (a 60 ms sample at n = 512 read 864 k evals/s where 100 ms read 980 k)
                eps2 = max(20000, ((1 << 28) // (2 * n2)) // 10)
                m2 = crs_measure(nlopt_amd, L, "rastrigin", n2, 100000, a.seed, 1, 10, eps2, sync_all)
                s0, s1 = m2["st0"], m2["st1"]
                gms, gb, gl = s1["t_gather_ms"] - s0["t_gather_ms"], s1["gather_bytes"] - s0["gather_bytes"], s1["gather_launches"] - s0["gather_launches"]
                e2 = {"workload": "NLOPT_GN_CRS2_LM rastrigin n=%d pop=100000 seed=%d, 10 steps of %d evals = one batch of stream blocks" % (n2, a.seed, eps2),
                      "value": m2["evals"] / m2["dt"], "unit": "evals/s",
                      "roofline_frac": (gb / 1e9) / (gms / 1e3) / HBM_PEAK_GBS if gms > 0 else None,
                      "avg_launch_ms": gms / gl if gl else None, "algorithmic_bytes_per_trial": 8 * n2 * (n2 + 1),
                      "init_evals_per_s": 100000 / m2["t_init"],
                      "path": "device-resolved windows (crs_chain_kernel, the chain advanced by the resolver wavefront): every dimension since round 5",
                      "trials_consumed_per_pass": (s1["slots_used"] - s0["slots_used"]) / max(1, s1["rounds"] - s0["rounds"]),
                      "host_split": {"trial_s": s1["t_trial_s"] - s0["t_trial_s"], "engine_s": s1["t_engine_s"] - s0["t_engine_s"],
                                     "walk_s": s1["t_walk_s"] - s0["t_walk_s"], "gather_kernel_s": gms / 1e3, "passes": int(s1["rounds"] - s0["rounds"]),
                                     "list_refreshes": int(s1["list_refreshes"] - s0["list_refreshes"]),
                                     "list_refreshes_beside_device": int(s1["list_refreshes_beside_device"] - s0["list_refreshes_beside_device"]),
                                     "list_refresh_s": s1["t_list_refresh_s"] - s0["t_list_refresh_s"]}}
                if not a.no_cpu_baseline:
                    cb = cpu_baseline_crs("rastrigin", n2, 20000, 4000, a.seed)
                    e2["cpu_baseline"] = cb
                    if cb.get("value"):
                        e2["speedup_vs_cpu_single_thread"] = e2["value"] / cb["value"]
                out["other_sizes"]["n=%d" % n2] = e2
            except Exception as e:
                out["other_sizes"]["n=%d" % n2] = {"error": repr(e)}
    if world > 1:
        if sharded:
            out["one_job"] = {"ranks": headline_one_job["ranks"], "init_wall_s": t_init, "allgather_bytes_timed": int(st1["allgather_bytes"] - st0["allgather_bytes"]),
                              "passes_timed": int(st1["rounds"] - st0["rounds"]),
                              "note": "value = the ONE job's rate (strong scaling); roofline = one rank's gather kernel on its column slice"}
        else:
            out["one_job"] = headline_one_job
            out["replicas_note"] = ("the one-job run failed (see one_job): value = sum over %d independent replicas of the metric configuration, scaling weak" % world)
        out["replicas"] = replicas
        out["config5_one_job"] = one_job
    if a.full:
        try:
            out["gens_to_ftol"] = gens_to_ftol()
        except Exception as e:        # the headline line must still be printed
            out["gens_to_ftol"] = {"error": repr(e)}
    if a.full and world == 1 and (n, pop, a.obj) == (4096, 100000, "griewank") and not a.headline_only:
        # SURVEY.md §8d defines the metric on nlopt_optimize(): one whole call (population initialisation included) on record
        try:
            out["nlopt_optimize_end_to_end"] = crs_end_to_end(nlopt_amd, a.obj, n, pop, a.seed, 20000)
        except Exception as e:
            out["nlopt_optimize_end_to_end"] = {"error": repr(e)}
        # BASELINE.json configs 3 and 4 in the same driver-run line (short: a few steps each), each with its own roofline and
        # cpu_baseline
        out["other_workloads"] = {}
        import copy
        for key, wl, steps, warm, exact in (("isres", "isres", 3, 1, False), ("mlsl", "mlsl", 2, 1, False), ("mlsl_exact_order", "mlsl", 2, 1, True)):
            try:
                b = copy.copy(a)
                b.workload, b.steps, b.warmup, b.exact = wl, steps, warm, exact
                b.n, b.pop, b.obj = {"isres": (256, 50000, "rastrigin"), "mlsl": (4096, 1000, "ackley")}[wl]
                b.local, b.cpu_sample_pop = "lbfgs", 0
                if exact:
                    b.no_cpu_baseline = True          # the same CPU run as the default mode's line
                out["other_workloads"][key] = bench_generational(b, nlopt_amd, L, 0, 1, None, sync_all, reduce)
                out["other_workloads"][key].pop("outputs")
            except (Exception, SystemExit) as e:
                out["other_workloads"][wl] = {"error": repr(e)}
    if a.full and not a.no_cpu_baseline and world == 1:       # the CPU baseline is timed on rank 0 of the 1-GPU run only
        try:
            # the headline's sample runs at the metric's OWN population (12 s of untimed reference initialisation at pop = 1e5, n = 4096;
            # round-5 verdict, weak 6: the rate had only ever been shown to be independent of pop on the survey's machine)
            out["cpu_baseline"] = cpu_baseline_crs(a.obj, n, a.cpu_sample_pop or (min(pop, 100000) if n >= 2048 else 20000), a.cpu_sample_trials, a.seed)
            if out["cpu_baseline"]["value"]:
                out["speedup_vs_cpu_single_thread"] = out["value"] / out["cpu_baseline"]["value"]
        except Exception as e:
            out["cpu_baseline"] = {"error": repr(e)}
    return out


def bench_generational(a, nlopt_amd, L, rank, world, dist, sync_all, reduce):
    """isres / mlsl: K generations of ONE nlopt_optimize() call, bracketed by the generation hook"""
    import _oracle as O
    n, pop, W, K = a.n, a.pop, a.warmup, a.steps
    xs, lo, hi = O.golden_x0(a.obj, n)
    comm = None
    if a.workload == "isres":
        o = nlopt_amd.Opt(nlopt_amd.GN_ISRES, n)
        ncon = 4
    elif a.local == "mma":
        o = nlopt_amd.Opt(nlopt_amd.GD_MLSL_LDS, n)             # no local optimiser set: the dispatcher's default, LD_MMA
        o.set_ftol_rel(1e-8)                                     # copied to the default local optimiser (optimize.c:772)
    else:
        o = nlopt_amd.Opt(nlopt_amd.G_MLSL_LDS, n)
        loc = nlopt_amd.Opt(nlopt_amd.LD_LBFGS, n)
        loc.set_ftol_rel(1e-8)
        if getattr(a, "exact", False):
            loc.set_param("amd_exact_dot", 1)
        L.nlopt_set_local_optimizer(o._h, loc._h)
    o.set_lower_bounds(lo)
    o.set_upper_bounds(hi)
    o.set_min_objective(nlopt_amd.objective(a.obj))
    o.set_population(pop)
    for kv in getattr(a, "param", []) or []:
        o.set_param(kv.split("=", 1)[0], float(kv.split("=", 1)[1]))
    if a.workload == "isres":
        o.add_blocksum_constraints(ncon, 1e-8)
    if world > 1:
        comm = nlopt_amd.Comm.from_torch_distributed()       # nccl group -> the library's own RCCL communicator
        o.set_comm(comm)
    marks = {}

    def hook(gens_done, numevals):
        if gens_done == W or gens_done == W + K:
            sync_all()
            marks[gens_done] = (time.perf_counter(), numevals, o.stats())
            if gens_done == W + K:
                o.force_stop()
    o.set_progress(hook)
    if a.workload == "mlsl":
        o.enable_trace((W + K + 2) * (pop + 4096))          # per local search: its start, minimum and evaluation count (the pin against the reference; the latency model below)
    nlopt_amd.srand(a.seed)                                   # every rank: the same stream (one job)
    t_start = time.perf_counter()
    x, minf, ret = o.optimize_raw(xs)
    t_total = time.perf_counter() - t_start
    if W not in marks or W + K not in marks:
        raise SystemExit("bench.py: the run ended before %d generations (result %d: %s)" % (W + K, ret, o.get_errmsg()))
    (t0, ev0, st0), (t1, ev1, st1) = marks[W], marks[W + K]
    dt_max, evals_all = reduce(t1 - t0, ev1 - ev0, False)
    if rank != 0:
        return None
    d = {k: st1[k] - st0[k] for k in st1}
    roof_extra = None
    if a.workload == "isres":
        # HBM side: what a generation must move algorithmically is 40 n bytes per candidate (eval 8n + evolve 16n read + 16n
        # written) over the eval + evolve passes actually executed (ev2_* kernels incl. their deviates' words)
        t_dom = d["t_eval_s"] + d["t_evolve_s"]
        bytes_dom = 40.0 * n * pop * K
        kern, launches = "isres_eval_kernel + ev2_stage/scan/chain/write_kernel (eval + evolve passes)", K
        # the DOMINANT kernel is not bandwidth-bound at all: the stochastic ranking is a systolic pipeline whose cost is its
        # serial tick chain (pop + 2 sweeps + 63 ceil(sweeps/64) ticks per launch): bound = latency
        if d.get("stochrank_launches"):
            ticks = float(d["stochrank_ticks"])
            t_sr = d["t_stochrank_ms"] / 1e3
            steps = float(d["rank_sweeps"]) * (pop - 1)
            roof_extra = {"bound": "latency", "kernel": "isres_stochrank_kernel", "launches": int(d["stochrank_launches"]),
                          "avg_launch_ms": d["t_stochrank_ms"] / d["stochrank_launches"],
                          "serial_ticks_per_launch": ticks / d["stochrank_launches"],
                          "achieved": t_sr * 1e9 / ticks if ticks else None, "unit": "ns per serial tick",
                          "model": "ticks = pop + 2*sweeps + 63*ceil(sweeps/64) (782 units of 64 sweeps in a row; the units hand over through the elements themselves); one tick = one DPP lane shift + compare-exchange of the "
                                   "packed element on a wavefront that is alone on its SIMD (26 VALU/DPP instructions, isres_kernels.hip)",
                          "peak": 26 * 4 / 2.4, "peak_note": "26 instructions x 4 cycles each (wave64 on a 16-lane SIMD) at 2.4 GHz = 43 ns: the floor of this formulation",
                          "frac": (26 * 4 / 2.4) / (t_sr * 1e9 / ticks) if ticks and t_sr > 0 else None,
                          "ranking_steps_per_s": steps / t_sr if t_sr > 0 else None,
                          "share_of_generation": t_sr / (dt_max) if dt_max > 0 else None,
                          "traffic": pmc_traffic("isres_stochrank_kernel")[0] if (n, pop, a.obj) == (256, 50000, "rastrigin") else None}
        metric = "candidate-evals/sec, ISRES n=%d pop=%d, %d inequality constraints" % (n, pop, ncon)
        wl = "NLOPT_GN_ISRES %s n=%d pop=%d + %d block-sum inequality constraints, seed=%d; step = 1 generation" % (a.obj, n, pop, ncon, a.seed)
        phases = {"eval_s_per_gen": d["t_eval_s"] / K, "rank_s_per_gen": d["t_rank_s"] / K, "evolve_s_per_gen": d["t_evolve_s"] / K,
                  "rng_s_per_gen_inside_rank_and_evolve": d["t_rng_s"] / K, "rank_sweeps_per_gen": d["rank_sweeps"] / K, "evolve_rounds_per_gen": d["evolve_rounds"] / K,
                  "evolve_rounds_enqueued_per_gen": d["evolve_rounds_enqueued"] / K,
                  # isres_driver.c "amd_isres_overlap": the generator on a stream of its own beside the latency-bound kernels (the
                  # default; --param amd_isres_overlap=0 gives the one-stream generation: 72.9 vs 65.3 ms, profiles/r03_isres_overlap_ab.txt)
                  "generator_on_its_own_stream": not any(kv.replace(" ", "") in ("amd_isres_overlap=0", "amd_isres_overlap=0.0") for kv in (getattr(a, "param", []) or []))}
    else:
        t_dom = d["t_lbfgs_ms"] / 1e3
        bytes_dom = float(d["lbfgs_bytes"])
        # the kernel the searches run on: the resident one up to n = 4096 with a device objective (hip/lbfgs_resident.hip), else the streaming one
        kern, launches = ("mma_batch_kernel" if a.local == "mma" else ("lbfgs_batch_kernel" if (n > 8192 or any(q.startswith("amd_lbfgs_streaming=") and float(q.split("=", 1)[1]) != 0 for q in a.param)) else ("lbfgs_resident_kernel" if n <= 4096 else "lbfgs_resident32_kernel"))), int(d["lbfgs_launches"])
        name = "GD_MLSL_LDS + default LD_MMA" if a.local == "mma" else "G_MLSL_LDS + LD_LBFGS"
        metric = "candidate-evals/sec, %s n=%d, %d samples per iteration" % (name, n, pop)
        mode = ("amd_exact_dot=1: every sum of the local search in the reference's sequential order, iterates bit-identical to the reference's"
                if getattr(a, "exact", False) else "default mode: workgroup tree sums in the local search, iterates equal to the reference's to rounding")
        wl = "NLOPT_%s(ftol_rel 1e-8) %s n=%d, %d samples/iteration, seed=%d; %s; step = 1 MLSL iteration" % (name.replace(" + ", " + NLOPT_").replace("default ", ""), a.obj, n, pop, a.seed, mode)
        phases = {"sampling_s_per_iter": d["t_eval_s"] / K, "local_phase_s_per_iter": d["t_evolve_s"] / K,
                  "local_searches": int(d["accepted"]), "sample_evals": int(d["evals_trial"]), "local_evals": int(d["evals_mutation"])}
    if a.workload == "mlsl" and getattr(a, "exact", False) and a.local == "lbfgs":
        # amd_exact_dot = 1 is not a bandwidth problem: every dot product of a search is ONE chain of n dependent fp64 additions in the
        # reference's order (mssubs.c:601-641), and a launch lasts as long as its longest search.  Steps of a search, counted by the library from
        # what the kernel reports per search (include/nlopt_amd.h, lbfgs_longest_chain_steps): n (2 cols + 4 nevals) — two dot products per
        # history column used, about four passes of ordered sums per evaluation.  (Rounds 2-5 modelled the steps from the evaluation counts
        # alone — adds(E) = n sum_{i<E} (2 min(i, mf) + 6) — which counts 5 times the columns the searches really use: the "2.5 ns per
        # addition" of those rounds was 9.6 ns of two v_readlane + v_add_f64 per step, tools/fmac_chain_probe.hip.)
        # floor: one step of a chain of dependent v_fmac_f64 with a row_newbcast operand, one wavefront per SIMD, measured alone on this
        # part: 3.2 ns (profiles/r06_fmac_chain_probe.txt; 4.9 ns with two such workgroups per compute unit, which 44 of 256 CUs carry).
        steps = float(d.get("lbfgs_longest_chain_steps", 0))
        if steps > 0 and t_dom > 0:
            ns = 1e9 * t_dom / steps
            roof_extra = {"bound": "latency", "kernel": kern, "launches": launches, "avg_launch_ms": 1e3 * t_dom / launches if launches else None,
                          "achieved": ns, "unit": "ns per step of the longest search's chain of dependent fp64 additions",
                          "peak": 3.2, "peak_note": "one dependent v_fmac_f64 (DPP row_newbcast operand) per step, one wavefront per SIMD, measured alone: tools/fmac_chain_probe.hip, profiles/r06_fmac_chain_probe.txt",
                          "frac": 3.2 / ns, "chain_steps_longest_search_per_launch": steps / launches if launches else None,
                          "model": "steps = n (2 cols + 4 nevals) of the launch's longest search (cols = history columns it streamed); launch time = its longest search",
                          "traffic": None}
    achieved = (bytes_dom / 1e9) / t_dom if t_dom > 0 else None
    # HBM bytes per launch of the dominant kernel from the committed PMC passes of the same command (BASELINE's shapes only)
    std = (a.workload == "isres" and (n, pop, a.obj) == (256, 50000, "rastrigin")) or (a.workload == "mlsl" and (n, pop, a.obj) == (4096, 1000, "ackley"))
    # (the PMC passes on record are of the default summation mode)
    traffic_dom, traffic_src = pmc_traffic(kern.split(" ")[0].split("<")[0]) if (std and a.workload == "mlsl" and not getattr(a, "exact", False)) else (None, None)
    out = {
        "metric": metric, "value": evals_all / dt_max, "unit": "evals/s", "n_gpus": world, "steps": K, "warmup": W,
        "ms_per_step": 1e3 * dt_max / K, "higher_is_better": True, "scaling": "strong" if world > 1 else "weak", "vs_baseline": None,
        "dtype": "f64", "data": "synthetic",
        "config": {"workload": wl + ("" if world == 1 else "; ONE job over %d ranks (library communicator over RCCL)" % world),
                   "evals_timed": int(evals_all)},
        "roofline": {"bound": "hbm", "kernel": kern, "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": (achieved / HBM_PEAK_GBS) if achieved else None, "traffic": traffic_dom, "traffic_source": traffic_src,
                     "launches": launches,
                     "avg_launch_ms": 1e3 * t_dom / launches if launches else None,
                     "avg_algorithmic_bytes_per_launch": bytes_dom / launches if launches else None},
        "phases": phases, "total_seconds_incl_setup": t_total, "final_result": int(ret), "minf": minf,
        "outputs": {"x": x, "minf": minf, "numevals": o.get_numevals()},
    }
    if a.full and world == 1:
        try:
            if a.workload == "isres":
                out["pinned_run"] = pinned_isres(n, pop, a.obj, a.seed, ncon, o.get_numevals(), minf, o.stats()["mt_words"])
            elif a.local == "lbfgs":
                out["pinned_run"] = pinned_mlsl(n, pop, a.obj, a.seed, bool(getattr(a, "exact", False)), W + K, o.get_numevals(), minf, o.trace())
        except Exception as e:
            out["pinned_run"] = {"error": repr(e)}
    if a.workload == "mlsl" and d.get("mlsl_sampled_ahead"):
        # round 5: the next iteration's sampling phase (points, values, pair distances: fp64-arithmetic-bound) runs BESIDE the searches' launch
        # (mlsl_driver.c, mlsl_enqueue_ahead): the iteration is shorter, the launch itself longer than alone (6.0 -> 7.4 ms on one box)
        out["roofline"]["co_running"] = "next iteration's mlsl_dist2_kernel (fp64-bound); alone: frac 0.25-0.29, r05_mlsl_ahead_ab.txt"
        out["phases"]["iterations_sampled_ahead"] = int(d["mlsl_sampled_ahead"])
    if roof_extra is not None:
        # the line's `roofline` names the dominant kernel; the HBM-side figure of the passes that do move data is kept beside it
        out["roofline_hbm_passes"] = out["roofline"]
        out["roofline"] = roof_extra
    if comm is not None:
        out["collectives"] = comm.counters()
    if a.full and not a.no_cpu_baseline and world == 1:
        try:
            if a.workload == "isres":
                out["cpu_baseline"] = cpu_baseline_isres(a.obj, n, a.cpu_sample_pop or pop, a.seed, ncon)
                if out["cpu_baseline"]["sample_pop"] != pop:
                    out["cpu_baseline"]["estimate_at_benchmark_pop"] = out["cpu_baseline"]["value"] * out["cpu_baseline"]["sample_pop"] / pop
            else:
                out["cpu_baseline"] = cpu_baseline_mlsl(a.obj, n, pop, a.seed, 30000, a.local)
            if out["cpu_baseline"]["value"]:
                out["speedup_vs_cpu_single_thread"] = out["value"] / out["cpu_baseline"]["value"]
        except Exception as e:
            out["cpu_baseline"] = {"error": repr(e)}
    return out


if __name__ == "__main__":
    main()
