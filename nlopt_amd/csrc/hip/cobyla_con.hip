/* cobyla_con.hip — batched NLOPT_LN_COBYLA with NONLINEAR CONSTRAINTS whose values come from outside this library (a user's device
 * constraint blocks, include/nlopt_amd_device.h), for an objective that comes from outside too: the coroutine of cobyla_ext.hip
 * (cw_search<0, 2>, one wavefront per start point, storage and protocol of "External evaluation" in include/nlopt_amd.h) with CON = 1.
 * At the one evaluation point the caller evaluates, beside the objective, every constraint block at row `inst` of EX and leaves the
 * values in row `inst` of EC: mi inequality values, then me equality values.  The search takes them as the first mc = mi + 2 me rows of
 * its linear programme, in front of the bound rows, exactly as the reference's func_wrap hands them to cobyla (cobyla.c:105-125): an
 * inequality row is -g, an equality block its values +h followed by the same block's -h.  Which column of EC a row reads and with
 * which sign is a table of mc ints from the caller (`rowmap`: c >= 0: +EC[c]; c < 0: -EC[-c - 1]), so the kernel knows nothing of
 * blocks.  tol (mi + me doubles, by column) enters the feasibility test in front of the stop-value check only (cobyla.c:598); the
 * greatest violation ignores it.  The result is the algorithm's own point and value: the reference memoizes the best point seen for
 * an unconstrained run only (optimize.c:485-506).
 *
 * Memory model: as cobyla_ext.hip.  EC, tol and rowmap are read-only in the kernel; EC was written by the caller's kernels between
 * two launches on the same stream, which is what makes it visible.
 *
 * Layout.  The row count is m = mc + (finite bounds) <= 2n + mc.  The slice is cw_global_doubles(n, 2n + mc) doubles, the save record
 * cw_save_doubles_con(n, mc), the LDS block cw_vec_doubles(n, 2n + mc) doubles: what serves is 8 x that <= 64 KiB (n = 256: mc <= 175;
 * n = 8: mc <= 1200).
 *
 * Bound by: what bounds cobyla_ext.hip's step — the iteration of the global instance, now over m rows (the model gradients are
 * (m + 1) n sums of length n, the LP's residual loops run over m), the record out and in, one launch — plus the caller's constraint
 * launches, one per block and step. */
#include "cobyla_search.h"

__global__ __launch_bounds__(CW_LANES) void cobyla_batch_ext_con_kernel(int n, int ld, int count, const double *__restrict__ lb, const double *__restrict__ ub,
                                                                        const double *__restrict__ dx_given, double *__restrict__ X, double *work, size_t slice,
                                                                        nla_cobyla_params P, nla_lbfgs_result *__restrict__ out, nla_local_ext E, cw_user_rows U)
{
#ifndef NLA_SIMT_EMU
    extern __shared__ double cw_lds[];
#endif
    __shared__ lb_shared S;
    __shared__ double oscratch[8];                   /* (the objective's buffers: this instance never touches them) */
    __shared__ lb_exact_buf XB;
    cw_search<0, 2, 1>(n, ld, count, lb, ub, dx_given, X, P, out, cw_lds, work + (size_t) blockIdx.x * slice, S, oscratch, XB, E, U);
}

#define CW_CON_LDS_MAX ((size_t) 64 * 1024)
static size_t cw_con_slice_doubles(int n, int mc) { return cw_global_doubles(n, 2 * n + mc); }
extern "C" int nla_cobyla_con_serves(int n, int mc)
{
    /* (mc bounded first: the sizes below are sums of ints) */
    return n >= 1 && n <= NLA_COBYLA_GLOBAL_MAX_N && mc >= 1 && mc <= 8192 && sizeof(double) * cw_vec_doubles(n, 2 * n + mc) <= CW_CON_LDS_MAX;
}
extern "C" size_t nla_cobyla_con_work_doubles(int n, int mc, int count)
{
    if (!nla_cobyla_con_serves(n, mc)) return 0;
    return cw_con_slice_doubles(n, mc) * (size_t) (count > 0 ? count : 1) + 16;
}
extern "C" size_t nla_cobyla_con_save_bytes(int n, int mc) { return nla_cobyla_con_serves(n, mc) ? sizeof(double) * cw_save_doubles_con(n, mc) : 0; }

extern "C" int nla_k_cobyla_batch_ext_con(int n, int ld, int count, const double *lb, const double *ub, const double *dx, double *X,
                                          double *work, const nla_cobyla_params *params, nla_lbfgs_result *out, const nla_local_ext *ext,
                                          int mi, int me, int ldc, const double *EC, const double *tol, const int32_t *rowmap, void *stream)
{
    if (count <= 0) return 0;
    if (mi < 0 || me < 0 || mi > 8192 || me > 8192 || !nla_cobyla_con_serves(n, mi + 2 * me) || ld < n || ldc < mi + me || !work || !params || !out || !X || !lb ||
        !ub || !ext || !ext->req || !ext->EX || !ext->EF || !ext->save || !EC || !tol || !rowmap) return (int) hipErrorInvalidValue;
    hipStream_t st = (hipStream_t) stream;
    nla_cobyla_params P = *params;
    nla_local_ext E = *ext;
    cw_user_rows U;
    const int mc = mi + 2 * me;
    P.abort = nullptr; P.done = nullptr;             /* the coroutine's stops are ext->forced / ext->timeout, its end req[].state = 2 */
    U.mc = mc; U.ldc = ldc; U.EC = EC; U.tol = tol; U.map = rowmap;
    const size_t lds = sizeof(double) * cw_vec_doubles(n, 2 * n + mc), slice = cw_con_slice_doubles(n, mc);
    double *base = (double *) (((uintptr_t) work + 127) & ~(uintptr_t) 127);
#ifndef NLA_SIMT_EMU
    if (lds > 48 * 1024) {
        hipError_t e_ = hipFuncSetAttribute((const void *) cobyla_batch_ext_con_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
        if (e_ != hipSuccess) return (int) e_;
    }
#endif
    hipLaunchKernelGGL(cobyla_batch_ext_con_kernel, dim3(count), dim3(CW_LANES), lds, st, n, ld, count, lb, ub, dx, X, base, slice, P, out, E, U);
    NLA_LAUNCH_CHECK();
    return 0;
}
