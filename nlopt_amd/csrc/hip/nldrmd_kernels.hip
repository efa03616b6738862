/* nldrmd_kernels.hip — batched NLOPT_LN_NELDERMEAD: replaces nldrmd_minimize with psi = 0 (src/algs/neldermead/nldrmd.c:290-314 over
 * nldrmd_minimize_, :106-288) as nlopt_optimize reaches it (optimize.c:886-905) for `count` independent starts at once, one WAVEFRONT per
 * start (one wavefront per workgroup, as the COBYLA kernels: a launch spreads thousands of searches over the compute units).  The search
 * body exists once (nm_search, hip/nm_search.h: NLOPT_LN_SBPLX's kernels run the same steps with psi > 0) and is instantiated
 *   nldrmd_batch_kernel<OBJ>   for a compiled-in device objective: the whole search is one launch;
 *   nldrmd_batch_ext_kernel    as a COROUTINE by the "External evaluation" contract of include/nlopt_amd.h: a launch runs every search
 *                              from where it stands to its next evaluation — the point goes to row `inst` of EX, req[inst] = {1, 0} — or
 *                              to its end (req[inst].state = 2) and ENDS; the caller evaluates, writes EF and launches again with
 *                              resume = 1.  want_grad is always 0, EF[inst] is taken as delivered, ext->forced / ext->timeout stand where
 *                              the reference's CHECK_EVAL asks nlopt_stop_forced / nlopt_stop_time, a finished search stays finished
 *                              through later launches, and a launch waits for nothing.
 *
 * Mapping.  Every coordinate loop of Nelder-Mead is independent per coordinate: lane l owns coordinates l, l + 64, ... of every point, in
 * every loop, so a lane only ever reads coordinates it wrote itself and each result is the reference's bit for bit with no cross-lane
 * sum.  What does cross lanes: the order of the simplex (comparisons only), the wave-wide ANDs of reflectpt, the two norms of the x-stop
 * test (summed in ascending coordinate order by every lane from LDS) and the objective.
 *
 * Storage.  The simplex — n + 1 rows of n coordinates — and the initial steps (one more row) live in the search's slice of `work`: rows
 * nm_ld(n) doubles apart, a whole number of 128-byte lines, the slice on a 128-byte boundary, so lane j reading coordinate j of a row is
 * one coalesced access.  The n + 1 function values, the centroid, the trial point and the point under evaluation live in LDS (4n + 1
 * doubles).  Between two launches of the coroutine those vectors and the live scalars (nm_saved) lie in the search's record of
 * ext->save; the slice and row `inst` of X (the best point seen, as the reference keeps it in x) are in device memory anyway.  A slice and
 * a record belong to ONE wavefront; what one launch stored the next reads across the kernel boundary: no fence, no atomic, no flag.
 *
 * Bound by: per iteration one or two passes over the (n + 1) n doubles of the simplex (a few KB at n <= 16: L2 / L1 hits), their load
 * latency in the n + 1 dependent additions of the centroid, and, for the coroutine, one kernel launch plus the record out and in per
 * evaluation — latency and launches, not bandwidth.  No scratch memory, no private arrays: the per-lane state is a handful of doubles.
 *
 * Out of scope: LN_NELDERMEAD as MLSL's local optimiser (mlsl_check_args keeps
 * its message), multi-rank batches, n > NLA_NLDRMD_MAX_N = 256.  A NaN objective value is outside the parity contract: the search still
 * ends at maxeval and disturbs no other search. */
#include "nm_search.h"            /* the search body (nm_search), shared with hip/sbplx_kernels.hip */

#ifdef NLA_SIMT_EMU
static double nm_lds[4 * NLA_NLDRMD_MAX_N + 1];                   /* (the CPU emulation runs one workgroup at a time) */
#endif

template <int OBJ>
__global__ __launch_bounds__(CW_LANES) void nldrmd_batch_kernel(int n, int ld, int count, const double *__restrict__ lb, const double *__restrict__ ub,
                                                                const double *__restrict__ dx_given, double *__restrict__ X, double *work,
                                                                size_t slice, nla_nldrmd_params P, nla_lbfgs_result *__restrict__ out)
{
#ifndef NLA_SIMT_EMU
    extern __shared__ __attribute__((aligned(16))) double nm_lds[];
#endif
    __shared__ lb_shared S;
    __shared__ double oscratch[8];
    __shared__ lb_exact_buf XB;
    nm_search<OBJ, false>(n, ld, count, lb, ub, dx_given, X, P, out, nm_lds, work + (size_t) blockIdx.x * slice, S, oscratch, XB);
}

__global__ __launch_bounds__(CW_LANES) void nldrmd_batch_ext_kernel(int n, int ld, int count, const double *__restrict__ lb, const double *__restrict__ ub,
                                                                    const double *__restrict__ dx_given, double *__restrict__ X, double *work,
                                                                    size_t slice, nla_nldrmd_params P, nla_lbfgs_result *__restrict__ out, nla_local_ext E)
{
#ifndef NLA_SIMT_EMU
    extern __shared__ __attribute__((aligned(16))) double nm_lds[];
#endif
    __shared__ lb_shared S;
    __shared__ double oscratch[8];                   /* (the objective's buffer: this instance never touches it) */
    __shared__ lb_exact_buf XB;                      /* (the x-stop test's ordered sums) */
    nm_search<0, true>(n, ld, count, lb, ub, dx_given, X, P, out, nm_lds, work + (size_t) blockIdx.x * slice, S, oscratch, XB, E);
}

extern "C" int nla_nldrmd_serves(int n) { return n >= 1 && n <= NLA_NLDRMD_MAX_N; }
/* 16 doubles more for the launcher to start the first slice on a 128-byte boundary wherever `work` starts */
extern "C" size_t nla_nldrmd_work_doubles(int n, int count)
{
    if (!nla_nldrmd_serves(n)) return 0;
    return nm_slice_doubles(n) * (size_t) (count > 0 ? count : 1) + 16;
}
extern "C" size_t nla_nldrmd_save_bytes(int n) { return nla_nldrmd_serves(n) ? sizeof(double) * nm_save_doubles(n) : 0; }

extern "C" int nla_k_nldrmd_batch(int obj, int n, int ld, int count, const double *lb, const double *ub, const double *dx, double *X,
                                  double *work, const nla_nldrmd_params *params, nla_lbfgs_result *out, const nla_local_ext *ext, void *stream)
{
    if (count <= 0) return 0;
    if (!nla_nldrmd_serves(n) || ld < n || !lb || !ub || !X || !work || !params || !out) return (int) hipErrorInvalidValue;
    if (obj == NLA_OBJ_EXTERNAL ? (!ext || !ext->req || !ext->EX || !ext->EF || !ext->save) : (obj < 0 || ext != nullptr)) return (int) hipErrorInvalidValue;
    hipStream_t st = (hipStream_t) stream;
    nla_nldrmd_params P = *params;
    if (P.sign == 0.) P.sign = 1.;
    const size_t lds = sizeof(double) * nm_vec_doubles(n), slice = nm_slice_doubles(n);      /* (at most 8.2 KB: no attribute to raise) */
    double *base = (double *) (((uintptr_t) work + 127) & ~(uintptr_t) 127);
    if (obj == NLA_OBJ_EXTERNAL) {
        nla_local_ext E = *ext;
        P.abort = nullptr; P.done = nullptr;         /* the coroutine's stops are ext->forced / ext->timeout, its end req[].state = 2 */
        hipLaunchKernelGGL(nldrmd_batch_ext_kernel, dim3(count), dim3(CW_LANES), lds, st, n, ld, count, lb, ub, dx, X, base, slice, P, out, E);
    } else {
#define CALL(O) hipLaunchKernelGGL((nldrmd_batch_kernel<O>), dim3(count), dim3(CW_LANES), lds, st, n, ld, count, lb, ub, dx, X, base, slice, P, out)
        NLA_OBJ_DISPATCH(obj, CALL)
#undef CALL
    }
    NLA_LAUNCH_CHECK();
    return 0;
}
