/* luksan_bounds.h — the bound handling Luksan's PLIS and PNET share (pssubs.c), by a workgroup of LB_T threads over thread-strided
 * coordinates: lbfgs_kernels.hip and tnewton_kernels.hip include it, so each loop exists once. */
#ifndef NLA_LUKSAN_BOUNDS_H
#define NLA_LUKSAN_BOUNDS_H
#include "local_common.h"
#include "../lbfgs_scalar.h"

__device__ __forceinline__ void lb_project(int n, double *x, const int *ix, const double *xl, const double *xu, double eps9)   /* pcbs04 */
{
    for (int i = threadIdx.x; i < n; i += LB_T) {
        const int t = ix[i] < 0 ? -ix[i] : ix[i];
        double v = x[i];
        if ((t == 1 || t == 3 || t == 4) && v <= xl[i] + eps9 * LB_MAX(fabs(xl[i]), 1.)) v = xl[i];
        if ((t == 2 || t == 3 || t == 4) && v >= xu[i] - eps9 * LB_MAX(fabs(xu[i]), 1.)) v = xu[i];
        x[i] = v;
    }
}
/* pyadc0; returns this thread's share of its inew: the coordinates that were free (ix > 0) and are on a bound now */
__device__ __forceinline__ int lb_add_active_count(int n, double *x, int *ix, const double *xl, const double *xu)
{
    int inew = 0;
    for (int i = threadIdx.x; i < n; i += LB_T) {
        const int ii = ix[i], t = ii < 0 ? -ii : ii;
        if (t >= 5) ix[i] = -t;
        else if ((t == 1 || t == 3 || t == 4) && x[i] <= xl[i]) { x[i] = xl[i]; ix[i] = (t == 4) ? -3 : -t; inew += ii > 0; }
        else if ((t == 2 || t == 3 || t == 4) && x[i] >= xu[i]) { x[i] = xu[i]; ix[i] = (t == 3) ? -4 : -t; inew += ii > 0; }
    }
    return inew;
}
__device__ __forceinline__ void lb_add_active(int n, double *x, int *ix, const double *xl, const double *xu) { (void) lb_add_active_count(n, x, ix, xl, xu); }

#endif
