/* cobyla_ext.hip — batched NLOPT_LN_COBYLA for an objective that is NOT compiled into this library (a user-supplied device objective,
 * include/nlopt_amd_device.h): the search of cobyla_kernels.hip / cobyla_global.hip (cobyla_search.h: one body for all three), one
 * wavefront per start point, as a COROUTINE around its one evaluation point (include/nlopt_amd.h "External evaluation").  A launch
 * runs every search of the batch from where it stands to its next evaluation — the point goes to row `inst` of EX, req[inst] = {1, 0} —
 * or to its end (req[inst].state = 2, X and out[inst] as the other two kernels leave them) and ENDS; the caller evaluates all waiting
 * points with one launch of the objective's kernel, writes EF and launches this kernel again with resume = 1.  The kernel waits for
 * nothing — no other workgroup, no stream, no host: a launch is a bounded piece of work (at most one iteration of every search).
 *
 * Memory model.  Storage as the global instance: the five matrices (SIM, SIMI, DAT, A, Z) in the search's slice of `work`, the vectors,
 * iact and rot in LDS.  Between two launches the LDS block and the scalars that are live across the evaluation (rho, parmu, the
 * counters, the repair generator's state ...: cw_saved) lie in the search's record of ext->save.  A slice and a save record belong to
 * ONE wavefront: what a lane stores, other lanes of that wavefront read behind the workgroup barrier; nothing is read across
 * workgroups.  What a launch stored — slice, record, req, EX — the next launch (and the objective's kernel between them, on the same
 * stream) reads across the kernel boundary, which is what makes it visible: no fence, no atomic, no flag in the kernel.
 *
 * Layout.  The slice: cw_global_doubles / cw_gld, as cobyla_global.hip (column-major, leading dimensions a whole, odd number of
 * 128-byte lines, the slice on a 128-byte boundary).  The record: cw_saved (15 doubles), then cw_vec_doubles(n, m) doubles of the LDS
 * block in its own order; records are cw_save_doubles(n) apart (sized for m = 2n, a multiple of 16 doubles).  The block moves
 * lane-strided both ways: coalesced.
 *
 * Bound by: per evaluation, the iteration of the global instance (L1 / L2 latency x the dependent fp64 adds of the serial sums) plus
 * the record out and in (2 x ~27 n doubles: 0.4 KB at n = 1, 110 KB at n = 256 — against the 3.9 MB slice the iteration walks) plus
 * one kernel launch; the caller's launch of the objective and its read-back of req stand beside it.  LDS 56 KB at n = 256. */
#include "cobyla_search.h"

__global__ __launch_bounds__(CW_LANES) void cobyla_batch_ext_kernel(int n, int ld, int count, const double *__restrict__ lb, const double *__restrict__ ub,
                                                                    const double *__restrict__ dx_given, double *__restrict__ X, double *work, size_t slice,
                                                                    nla_cobyla_params P, nla_lbfgs_result *__restrict__ out, nla_local_ext E)
{
#ifndef NLA_SIMT_EMU
    extern __shared__ double cw_lds[];
#endif
    __shared__ lb_shared S;
    __shared__ double oscratch[8];                   /* (the objective's buffers: this instance never touches them) */
    __shared__ lb_exact_buf XB;
    cw_search<0, 2>(n, ld, count, lb, ub, dx_given, X, P, out, cw_lds, work + (size_t) blockIdx.x * slice, S, oscratch, XB, E);
}

/* one search's slice: sized for a fully finite box (m = 2n rows) whatever the box, as the global instance's; 16 doubles more for the
 * launcher to start the first slice on a 128-byte boundary wherever `work` starts */
static size_t cw_ext_slice_doubles(int n) { return cw_global_doubles(n, 2 * n); }
static int cw_ext_fits(int n) { return n >= 1 && n <= NLA_COBYLA_GLOBAL_MAX_N; }
extern "C" size_t nla_cobyla_ext_work_doubles(int n, int count)
{
    if (!cw_ext_fits(n)) return 0;
    return cw_ext_slice_doubles(n) * (size_t) (count > 0 ? count : 1) + 16;
}
extern "C" size_t nla_cobyla_save_bytes(int n) { return cw_ext_fits(n) ? sizeof(double) * cw_save_doubles(n) : 0; }

extern "C" int nla_k_cobyla_batch_ext(int n, int ld, int count, const double *lb, const double *ub, const double *dx, double *X,
                                      double *work, const nla_cobyla_params *params, nla_lbfgs_result *out, const nla_local_ext *ext, void *stream)
{
    if (count <= 0) return 0;
    if (!cw_ext_fits(n) || ld < n || !work || !ext || !ext->req || !ext->EX || !ext->EF || !ext->save) return (int) hipErrorInvalidValue;
    hipStream_t st = (hipStream_t) stream;
    nla_cobyla_params P = *params;
    nla_local_ext E = *ext;
    P.abort = nullptr; P.done = nullptr;             /* the coroutine's stops are ext->forced / ext->timeout, its end req[].state = 2 */
    const size_t lds = sizeof(double) * cw_vec_doubles(n, 2 * n), slice = cw_ext_slice_doubles(n);
    double *base = (double *) (((uintptr_t) work + 127) & ~(uintptr_t) 127);
#ifndef NLA_SIMT_EMU
    if (lds > 48 * 1024) {
        hipError_t e_ = hipFuncSetAttribute((const void *) cobyla_batch_ext_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
        if (e_ != hipSuccess) return (int) e_;
    }
#endif
    hipLaunchKernelGGL(cobyla_batch_ext_kernel, dim3(count), dim3(CW_LANES), lds, st, n, ld, count, lb, ub, dx, X, base, slice, P, out, E);
    NLA_LAUNCH_CHECK();
    return 0;
}
