/* cobyla_kernels.hip — batched NLOPT_LN_COBYLA on gfx950: the local searches of NLOPT_GN_MLSL / GN_MLSL_LDS (whose default local
 * optimiser it is, src/api/optimize.c:763-768) with a compiled-in device objective, ONE WAVEFRONT per start point, the whole search
 * on the device and its whole state in LDS (rounds 2-5 ran these searches one after another on the host).
 *
 * What one search is (src/algs/cobyla/cobyla.c:181-271 around :452-1872, as nlopt_optimize reaches it through optimize.c:836-851):
 *   set-up     the default initial step from the start point and the box (options.c:921-946) unless the caller gave one; coordinates
 *              rescaled by the steps (rescale.c:30-48); the box as 2n linear constraint rows AND enforced on every point (cobyla.c:79-124);
 *              rhobeg = |dx_0 / scale_0|, rhoend from xtol_rel / xtol_abs
 *   iteration  Powell's COBYLA: linear models of f and of every row on a simplex of n+1 points (cobyla.c:688-811), a trust-region LP
 *              with an active set kept by Givens rotations (TRSTLP, cobyla.c:1247-1872), a merit function with an adaptive penalty
 *   result     the best point any evaluation saw (the dispatcher's memoize wrapper for unconstrained COBYLA, optimize.c:450-508,1026-1071)
 *
 * How the wavefront runs it.  The algorithm is a chain of small dense operations (n <= 51 here) whose every sum the reference forms
 * in one accumulator over ascending indices.  To stay the reference's run evaluation by evaluation that ORDER is kept; what is spread
 * over the 64 lanes is the set of independent sums and the element-wise updates:
 *   "map"      v[i] = ... for all i: lane-strided                                  (vertex / direction / multiplier updates)
 *   "many"     a SET of independent sums (the n^2 entries of SIMI x SIM - 1, the (m+1) n model gradients, the residuals of the inactive
 *              rows, the n rows of a rank-one update ...): one sum per lane, each lane serial over its own
 *   "one"      a single sum that decides the next step (a Givens angle, a multiplier): every lane forms it redundantly out of LDS
 *              (broadcast reads), so the value is in every lane's registers without an exchange
 *   "rows"     a CHAIN of Givens rotations over neighbouring columns of Z (adding a row to the active set, cobyla.c:1402-1448): the
 *              angles depend only on sums over columns no earlier rotation of the chain touches, so all angles come first ("many" +
 *              a scalar recurrence) and then every lane carries ONE ROW of Z through the whole chain
 * Scalars (rho, parmu, the LP's counters ...) live in every lane's registers, identical by construction; control flow is uniform.
 * Matrices are column-major with an ODD leading dimension: both the walk down a column and the walk along a row are free of LDS bank
 * conflicts.  Between two phases that touch the same array from different lanes stands a workgroup barrier (one wavefront: cheap).
 *
 * The same algorithm as ONE thread's state machine is ../cobyla_core.h (the host's LN_COBYLA, cobyla_host.c); the two are compared
 * evaluation by evaluation on the CPU (tools/cobyla_emu_check.py: this file compiled by g++ over tools/simt_emu, 64 lockstep threads)
 * and on the device against the real reference (tests/test_gpu_cobyla.py).
 *
 * The search itself is cobyla_search.h (cw_search), shared with cobyla_global.hip, which serves the dimensions beyond this file's with
 * the matrices in global memory; this file is the instance whose whole state is in LDS.
 *
 * Bound by: LDS latency x dependent fp64 adds of the serial sums; HBM and MFMA play no part (per evaluation: n doubles of the start /
 * result row).  Occupancy: LDS per search ~ (4n + m + 2)(n|1) + (n+1)((m+2)|1) + 14n + 8m doubles (n = 16: 22 KB, 7 searches per
 * compute unit; n = 40: 102 KB, one). */
#include "cobyla_search.h"

template <int OBJ>
__global__ __launch_bounds__(CW_LANES) void cobyla_batch_kernel(int n, int ld, int count, const double *__restrict__ lb, const double *__restrict__ ub,
                                                                const double *__restrict__ dx_given, double *__restrict__ X,
                                                                nla_cobyla_params P, nla_lbfgs_result *__restrict__ out)
{
#ifndef NLA_SIMT_EMU
    extern __shared__ double cw_lds[];
#endif
    __shared__ lb_shared S;
    __shared__ double oscratch[8];
    __shared__ lb_exact_buf XB;
    cw_search<OBJ, 0>(n, ld, count, lb, ub, dx_given, X, P, out, cw_lds, nullptr, S, oscratch, XB);
}

/* the searches keep their state in LDS: no workspace in global memory (the sizes stay in the interface for the allocation's sake) */
extern "C" size_t nla_cobyla_work_doubles(int n, int ld, int count) { (void) n; (void) ld; return (size_t) (count > 0 ? count : 1); }
extern "C" size_t nla_cobyla_work_ints(int n, int count) { (void) n; return (size_t) (count > 0 ? count : 1); }
/* bytes of LDS one search of n variables inside a fully finite box needs (m = 2n rows); the kernel serves n while this fits the
 * compute unit's 160 KB beside the fixed buffers */
extern "C" size_t nla_cobyla_lds_bytes(int n) { return sizeof(double) * cw_lds_doubles(n, 2 * n) + 2048; }
extern "C" int nla_cobyla_fits(int n) { return n >= 1 && nla_cobyla_lds_bytes(n) <= 160 * 1024; }

extern "C" int nla_k_cobyla_batch(int obj, int n, int ld, int count, const double *lb, const double *ub, const double *dx, double *X,
                                  double *work, int *iwork, const nla_cobyla_params *params, nla_lbfgs_result *out, void *stream)
{
    (void) work; (void) iwork;
    if (count <= 0) return 0;
    if (obj < 0 || n < 1 || ld < n || !nla_cobyla_fits(n)) return (int) hipErrorInvalidValue;
    hipStream_t st = (hipStream_t) stream;
    nla_cobyla_params P = *params;
    if (P.sign == 0.) P.sign = 1.;
    const size_t lds = sizeof(double) * cw_lds_doubles(n, 2 * n);
#ifdef NLA_SIMT_EMU
#define CALL(O) hipLaunchKernelGGL((cobyla_batch_kernel<O>), dim3(count), dim3(CW_LANES), lds, st, n, ld, count, lb, ub, dx, X, P, out)
#else
#define CALL(O) do { if (lds > 48 * 1024) { hipError_t e_ = hipFuncSetAttribute((const void *) cobyla_batch_kernel<O>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds); \
                                            if (e_ != hipSuccess) return (int) e_; } \
                     hipLaunchKernelGGL((cobyla_batch_kernel<O>), dim3(count), dim3(CW_LANES), lds, st, n, ld, count, lb, ub, dx, X, P, out); } while (0)
#endif
    NLA_OBJ_DISPATCH(obj, CALL)
#undef CALL
    NLA_LAUNCH_CHECK();
    return 0;
}

