/* sbplx_kernels.hip — batched NLOPT_LN_SBPLX: replaces sbplx_minimize (src/algs/neldermead/sbplx.c:66-237) over nldrmd_minimize_ with
 * psi = 0.25 (nldrmd.c:106-288) as nlopt_optimize reaches it (optimize.c:886-905) for `count` independent starts at once, one WAVEFRONT
 * per start and one wavefront per workgroup, as hip/nldrmd_kernels.hip.  The search body is nm_search<.., SB = true> of hip/nm_search.h —
 * the Nelder-Mead steps there exist once for both algorithms — and is instantiated
 *   sbplx_batch_kernel<OBJ>   for a compiled-in device objective: the whole search is one launch;
 *   sbplx_batch_ext_kernel    as a COROUTINE by the "External evaluation" contract of include/nlopt_amd.h: a launch runs every search from
 *                             where it stands to its next evaluation — the FULL point goes to row `inst` of EX, req[inst] = {1, 0} — or to
 *                             its end (req[inst].state = 2) and ENDS; the caller evaluates, writes EF and launches again with resume = 1.
 *                             ext->forced / ext->timeout stand where CHECK_EVAL asks, a finished search stays finished.
 *
 * Mapping.  The outer algorithm's vectors x, xprev, dx, xstep: lane l owns coordinates l, l + 64, ...  The permutation p (indices by
 * decreasing |dx|, ties in index order as glibc's stable qsort_r leaves them): lane l counts, for its coordinates i, the j with
 * |dx_j| > |dx_i| or (|dx_j| == |dx_i| and j < i) — comparisons only — and writes p[rank] = i.  The partition's sums (normdx, norm, normi,
 * goodness), the diameters of the sub-simplex and the scale's two norms are sequential sums in the reference's order, computed by EVERY
 * lane from LDS (uniform across the wave, never a tree).  In the Nelder-Mead steps lanes 0 .. ns - 1 own the subspace's coordinates.
 * The objective is evaluated over the full x by the whole wave (nla_block_objective_as / lb_obj_exact, selected by P.exact).
 *
 * Storage.  O(n) per search, all of it in LDS (sb_vec_doubles(n): 4 n doubles, the 112 doubles of the sub-simplex block, n ints; 10.1 KB
 * at n = 256).  `work` is not used.  Between two launches of the coroutine that block and the live scalars (sb_saved) lie in the search's
 * record of ext->save, a whole number of 128-byte lines; row `inst` of X is read at the start and written at the end.
 *
 * Bound by (expected, not measured in isolation): the objective's evaluation and the dependent LDS loads of the serial Nelder-Mead steps
 * on at most 6 x 5 doubles — latency, not bandwidth; per pass one O(n^2 / 64) rank count and three O(n) serial sums per lane, which at
 * n = 256 are a few thousand LDS reads against some 600 evaluations.  For the coroutine: one launch plus the record out and in per
 * evaluation.  No scratch memory, no VGPR spill, no private arrays (tests/test_sbplx_cpu.py reads the code object).
 *
 * Out of scope: n > NLA_SBPLX_MAX_N = 256, LN_SBPLX as MLSL's local optimiser, multi-rank batches, several searches per workgroup.  A
 * NaN objective value is outside the parity contract: the search still ends at maxeval and disturbs no other search. */
#include "nm_search.h"

#ifdef NLA_SIMT_EMU
static double sb_lds[4 * NLA_SBPLX_MAX_N + SB_SUB_DOUBLES + (NLA_SBPLX_MAX_N + 1) / 2];      /* (the CPU emulation runs one workgroup at a time) */
#endif

template <int OBJ>
__global__ __launch_bounds__(CW_LANES) void sbplx_batch_kernel(int n, int ld, int count, const double *__restrict__ lb, const double *__restrict__ ub,
                                                               const double *__restrict__ dx_given, double *__restrict__ X, nla_sbplx_params P,
                                                               nla_lbfgs_result *__restrict__ out)
{
#ifndef NLA_SIMT_EMU
    extern __shared__ __attribute__((aligned(16))) double sb_lds[];
#endif
    __shared__ lb_shared S;
    __shared__ double oscratch[8];
    __shared__ lb_exact_buf XB;
    nm_search<OBJ, false, true>(n, ld, count, lb, ub, dx_given, X, P, out, sb_lds, nullptr, S, oscratch, XB);
}

__global__ __launch_bounds__(CW_LANES) void sbplx_batch_ext_kernel(int n, int ld, int count, const double *__restrict__ lb, const double *__restrict__ ub,
                                                                   const double *__restrict__ dx_given, double *__restrict__ X, nla_sbplx_params P,
                                                                   nla_lbfgs_result *__restrict__ out, nla_local_ext E)
{
#ifndef NLA_SIMT_EMU
    extern __shared__ __attribute__((aligned(16))) double sb_lds[];
#endif
    __shared__ lb_shared S;
    __shared__ double oscratch[8];                   /* (the objective's buffer: this instance never touches it) */
    __shared__ lb_exact_buf XB;                      /* (the x-stop test's ordered sums) */
    nm_search<0, true, true>(n, ld, count, lb, ub, dx_given, X, P, out, sb_lds, nullptr, S, oscratch, XB, E);
}

extern "C" int nla_sbplx_serves(int n) { return n >= 1 && n <= NLA_SBPLX_MAX_N; }
/* nothing of a search lives in `work`: a token, so that the launcher's contract is LN_NELDERMEAD's */
extern "C" size_t nla_sbplx_work_doubles(int n, int count) { (void) count; return nla_sbplx_serves(n) ? 16 : 0; }
extern "C" size_t nla_sbplx_save_bytes(int n) { return nla_sbplx_serves(n) ? sizeof(double) * sb_save_doubles(n) : 0; }

extern "C" int nla_k_sbplx_batch(int obj, int n, int ld, int count, const double *lb, const double *ub, const double *dx, double *X,
                                 double *work, const nla_sbplx_params *params, nla_lbfgs_result *out, const nla_local_ext *ext, void *stream)
{
    if (count <= 0) return 0;
    if (!nla_sbplx_serves(n) || ld < n || !lb || !ub || !X || !work || !params || !out) return (int) hipErrorInvalidValue;
    if (obj == NLA_OBJ_EXTERNAL ? (!ext || !ext->req || !ext->EX || !ext->EF || !ext->save) : (obj < 0 || ext != nullptr)) return (int) hipErrorInvalidValue;
    hipStream_t st = (hipStream_t) stream;
    nla_sbplx_params P = *params;
    if (P.sign == 0.) P.sign = 1.;
    const size_t lds = sizeof(double) * sb_vec_doubles(n);       /* (at most 10.1 KB: no attribute to raise) */
    if (obj == NLA_OBJ_EXTERNAL) {
        nla_local_ext E = *ext;
        P.abort = nullptr; P.done = nullptr;         /* the coroutine's stops are ext->forced / ext->timeout, its end req[].state = 2 */
        hipLaunchKernelGGL(sbplx_batch_ext_kernel, dim3(count), dim3(CW_LANES), lds, st, n, ld, count, lb, ub, dx, X, P, out, E);
    } else {
#define CALL(O) hipLaunchKernelGGL((sbplx_batch_kernel<O>), dim3(count), dim3(CW_LANES), lds, st, n, ld, count, lb, ub, dx, X, P, out)
        NLA_OBJ_DISPATCH(obj, CALL)
#undef CALL
    }
    NLA_LAUNCH_CHECK();
    return 0;
}
