/* lbfgs_driver.c — NLOPT_LD_LBFGS behind the reference's entry point luksan_plis (plis.c:420-510):
 * argument handling on the host, the optimisation itself in the batched device kernel
 * (hip/lbfgs_kernels.hip) on the local optimisers' batch context (local_ctx.c) with count = 1; MLSL (mlsl_driver.c) and
 * nlopt_amd_optimize_batch (batch_driver.c) run the same kernel there with one workgroup per start point. */
#include "nla_internal.h"

#define MEMAVAIL 1310720                       /* luksan.h:149 */

int nla_lbfgs_default_mf(int n, int mf, int maxeval)        /* plis.c:441-445 */
{
    if (mf <= 0) {
        mf = MEMAVAIL / n > 10 ? MEMAVAIL / n : 10;
        if (maxeval > 0 && maxeval <= mf) mf = maxeval > 1 ? maxeval : 1;
    }
    return mf;
}

/* reference-shaped entry: luksan_plis(n, f, f_data, lb, ub, x, minf, stop, mf, tolg) (plis.c:420-426) */
nlopt_result nla_lbfgs_minimize(nlopt_opt opt, int n, nlopt_func f, void *f_data, const double *lb, const double *ub, double *x, double *minf,
                                nla_stopping *stop, int mf, double tolg)
{
    return nla_local_minimize_one(NLA_LOCAL_LBFGS, opt, n, f, f_data, lb, ub, x, minf, stop, nla_lbfgs_default_mf(n, mf, stop->maxeval), tolg, NULL, NULL);
}
