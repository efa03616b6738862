/* nldrmd_driver.c — NLOPT_LN_NELDERMEAD and NLOPT_LN_SBPLX behind the reference's entry points nldrmd_minimize
 * (src/algs/neldermead/nldrmd.c:290-314) and sbplx_minimize (sbplx.c:66-237) as nlopt_optimize reaches them (optimize.c:886-905).  The
 * whole search runs in the batched device kernel (hip/nldrmd_kernels.hip / hip/sbplx_kernels.hip, one wavefront per search) on the
 * context every local optimiser shares (local_ctx.c) with count = 1: one launch for a compiled-in device objective, the coroutine for a
 * user's device objective or an ordinary host callback (called on the caller's thread, one x at a time, in the reference's order).
 * There is no host twin: a lone search runs where the searches of a batch run, so search i of nlopt_amd_optimize_batch is this run bit
 * for bit.  The two drivers differ in the context's algorithm and in what a too-small starting step ends with, so they are one function.
 * Out of scope: either algorithm as MLSL's local optimiser, n > NLA_NLDRMD_MAX_N = NLA_SBPLX_MAX_N. */
#include "nla_internal.h"
#include <stdlib.h>

static nlopt_result minimize_as(int alg, nlopt_opt opt, int n, nlopt_func f, void *f_data, const double *lb, const double *ub, double *x,
                                double *minf, nla_stopping *stop)
{
    nla_lbfgs_result res = { 0., 0, 0, 0, 0 };
    nlopt_result ret;
    int freedx = 0;
    if (!opt->dx) {                                           /* optimize.c:891-903: the default step at the start point, forgotten afterwards */
        freedx = 1;
        if (nlopt_set_default_initial_step(opt, x) != NLOPT_SUCCESS) { nla_stop_msg(stop, "failed to allocate initial step"); return NLOPT_OUT_OF_MEMORY; }
    }
    ret = nla_local_minimize_one_res(alg, opt, n, f, f_data, lb, ub, x, minf, stop, 0, 0., NULL, opt->dx, &res);
    if (freedx) { free(opt->dx); opt->dx = NULL; }
    /* the simplex check (nldrmd.c:156-161): the kernel reports the dimension in the result record.  LN_NELDERMEAD: NLOPT_FAILURE.
     * LN_SBPLX: sbplx_minimize turns it into NLOPT_XTOL_REACHED (sbplx.c:162,183) and the reference's nlopt_stop_msg has left the message
     * all the same; the dimension is the subspace's, 1 + it in the record (0: no such end) */
    if (alg == NLA_LOCAL_NLDRMD ? ret == NLOPT_FAILURE && res.ret == NLOPT_FAILURE : ret == NLOPT_XTOL_REACHED && res.ret == NLOPT_XTOL_REACHED && res.cols > 0)
        nla_stop_msg(stop, "starting step size led to simplex that was too small in dimension %d", (int) res.cols - (alg == NLA_LOCAL_SBPLX));
    return ret;
}

nlopt_result nla_nldrmd_minimize(nlopt_opt opt, int n, nlopt_func f, void *f_data, const double *lb, const double *ub, double *x, double *minf,
                                 nla_stopping *stop)
{
    return minimize_as(NLA_LOCAL_NLDRMD, opt, n, f, f_data, lb, ub, x, minf, stop);
}

nlopt_result nla_sbplx_minimize(nlopt_opt opt, int n, nlopt_func f, void *f_data, const double *lb, const double *ub, double *x, double *minf,
                                nla_stopping *stop)
{
    return minimize_as(NLA_LOCAL_SBPLX, opt, n, f, f_data, lb, ub, x, minf, stop);
}
