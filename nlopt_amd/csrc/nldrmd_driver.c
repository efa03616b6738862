/* nldrmd_driver.c — NLOPT_LN_NELDERMEAD behind the reference's entry point nldrmd_minimize (src/algs/neldermead/nldrmd.c:290-314) as
 * nlopt_optimize reaches it (optimize.c:886-905).  The whole search runs in the batched device kernel (hip/nldrmd_kernels.hip, one
 * wavefront per search) on the context every local optimiser shares (local_ctx.c) with count = 1: one launch for a compiled-in device
 * objective, the coroutine for a user's device objective or an ordinary host callback (called on the caller's thread, one x at a time,
 * in the reference's order).  There is no host twin: a lone search runs where the searches of a batch run, so search i of
 * nlopt_amd_optimize_batch is this run bit for bit.
 * Out of scope: NLOPT_LN_SBPLX (nldrmd_minimize_ with psi > 0), LN_NELDERMEAD as MLSL's local optimiser, n > NLA_NLDRMD_MAX_N. */
#include "nla_internal.h"
#include <stdlib.h>

nlopt_result nla_nldrmd_minimize(nlopt_opt opt, int n, nlopt_func f, void *f_data, const double *lb, const double *ub, double *x, double *minf,
                                 nla_stopping *stop)
{
    nla_lbfgs_result res = { 0., 0, 0, 0, 0 };
    nlopt_result ret;
    int freedx = 0;
    if (!opt->dx) {                                           /* optimize.c:891-903: the default step at the start point, forgotten afterwards */
        freedx = 1;
        if (nlopt_set_default_initial_step(opt, x) != NLOPT_SUCCESS) { nla_stop_msg(stop, "failed to allocate initial step"); return NLOPT_OUT_OF_MEMORY; }
    }
    ret = nla_local_minimize_one_res(NLA_LOCAL_NLDRMD, opt, n, f, f_data, lb, ub, x, minf, stop, 0, 0., NULL, opt->dx, &res);
    if (freedx) { free(opt->dx); opt->dx = NULL; }
    /* the simplex check (nldrmd.c:156-161): the kernel reports the dimension in the result record */
    if (ret == NLOPT_FAILURE && res.ret == NLOPT_FAILURE)
        nla_stop_msg(stop, "starting step size led to simplex that was too small in dimension %d", (int) res.cols);
    return ret;
}
