/* cobyla_global.hip — batched NLOPT_LN_COBYLA beyond the dimension whose state fits a compute unit's LDS: the search of
 * cobyla_kernels.hip (cobyla_search.h: one body for both), one wavefront per start point, with its five matrices — the simplex SIM, its
 * inverse SIMI, the vertex values DAT, the model gradients A and the LP's basis Z, (4n + m + 2) n doubles and more — in a per-search
 * slice of a global-memory workspace and only the vectors, iact and rot (about 26 n doubles) in LDS.
 *
 * Memory model.  A slice belongs to one workgroup = one wavefront on one compute unit: what a lane stores, other lanes of the same
 * wavefront read behind the same workgroup barrier that orders the LDS instance's accesses (plain global loads and stores through that
 * compute unit's vector L1; nothing is read across workgroups).  The slice pointer is neither const nor restrict; the kernel zeroes
 * what it uses of the slice before the search, as the LDS instance zeroes its block.
 *
 * Layout.  Column-major like the LDS instance, the leading dimensions a whole, odd number of 128-byte lines (cw_gld), every slice on a
 * 128-byte boundary.  The two access shapes of the search: a lane walks down ITS column (the "many" sums: a new line every 16 steps, 64
 * live lines per wavefront = 8 KB of the 32 KB L1), or the lanes walk along a row / all read one element (coalesced / broadcast).
 *
 * Bound by: L1 / L2 latency x the dependent fp64 adds of the serial sums.  Footprint per search at n = 256: 3.9 MB (past the L1, in L2 /
 * HBM); LDS 56 KB. */
#include "cobyla_search.h"

template <int OBJ>
__global__ __launch_bounds__(CW_LANES) void cobyla_batch_global_kernel(int n, int ld, int count, const double *__restrict__ lb, const double *__restrict__ ub,
                                                                       const double *__restrict__ dx_given, double *__restrict__ X, double *work, size_t slice,
                                                                       nla_cobyla_params P, nla_lbfgs_result *__restrict__ out)
{
#ifndef NLA_SIMT_EMU
    extern __shared__ double cw_lds[];
#endif
    __shared__ lb_shared S;
    __shared__ double oscratch[8];
    __shared__ lb_exact_buf XB;
    cw_search<OBJ, 1>(n, ld, count, lb, ub, dx_given, X, P, out, cw_lds, work + (size_t) blockIdx.x * slice, S, oscratch, XB);
}

/* one search's slice: sized for a fully finite box (m = 2n rows) whatever the box; 16 doubles more for the launcher to start the
 * first slice on a 128-byte boundary wherever `work` starts */
static size_t cw_slice_doubles(int n) { return cw_global_doubles(n, 2 * n); }
extern "C" int nla_cobyla_global_fits(int n) { return n >= 1 && n <= NLA_COBYLA_GLOBAL_MAX_N; }
extern "C" size_t nla_cobyla_global_work_doubles(int n, int count)
{
    if (!nla_cobyla_global_fits(n)) return 0;
    return cw_slice_doubles(n) * (size_t) (count > 0 ? count : 1) + 16;
}

extern "C" int nla_k_cobyla_batch_global(int obj, int n, int ld, int count, const double *lb, const double *ub, const double *dx, double *X,
                                         double *work, int *iwork, const nla_cobyla_params *params, nla_lbfgs_result *out, void *stream)
{
    (void) iwork;
    if (count <= 0) return 0;
    if (obj < 0 || n < 1 || ld < n || !nla_cobyla_global_fits(n) || !work) return (int) hipErrorInvalidValue;
    hipStream_t st = (hipStream_t) stream;
    nla_cobyla_params P = *params;
    if (P.sign == 0.) P.sign = 1.;
    const size_t lds = sizeof(double) * cw_vec_doubles(n, 2 * n), slice = cw_slice_doubles(n);
    double *base = (double *) (((uintptr_t) work + 127) & ~(uintptr_t) 127);
#ifdef NLA_SIMT_EMU
#define CALL(O) hipLaunchKernelGGL((cobyla_batch_global_kernel<O>), dim3(count), dim3(CW_LANES), lds, st, n, ld, count, lb, ub, dx, X, base, slice, P, out)
#else
#define CALL(O) do { if (lds > 48 * 1024) { hipError_t e_ = hipFuncSetAttribute((const void *) cobyla_batch_global_kernel<O>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds); \
                                            if (e_ != hipSuccess) return (int) e_; } \
                     hipLaunchKernelGGL((cobyla_batch_global_kernel<O>), dim3(count), dim3(CW_LANES), lds, st, n, ld, count, lb, ub, dx, X, base, slice, P, out); } while (0)
#endif
    NLA_OBJ_DISPATCH(obj, CALL)
#undef CALL
    NLA_LAUNCH_CHECK();
    return 0;
}
