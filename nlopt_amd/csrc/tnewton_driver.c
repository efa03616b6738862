/* tnewton_driver.c — NLOPT_LD_TNEWTON, _RESTART, _PRECOND and _PRECOND_RESTART behind the reference's entry point luksan_pnet
 * (pnet.c:567-662): argument handling on the host, the optimisation itself — the CG iteration with its finite-difference
 * Hessian-vector products included — in the batched device kernel (hip/tnewton_kernels.hip) on the local optimisers' batch context
 * (local_ctx.c) with count = 1; nlopt_amd_optimize_batch (batch_driver.c) runs the same kernel there with one workgroup per start, so
 * search i of a batch is this run bit for bit.  The kernel returns the best point any evaluation saw inside the box, as the
 * reference's memoize_func does for these four algorithms (optimize.c:460-508).  Out of scope: MLSL's local phase. */
#include "nla_internal.h"

/* reference-shaped entry: luksan_pnet(n, f, f_data, lb, ub, x, minf, stop, mf, mos1, mos2, tolg) (pnet.c:567-574) */
nlopt_result nla_tnewton_minimize(nlopt_opt opt, int n, nlopt_func f, void *f_data, const double *lb, const double *ub, double *x, double *minf,
                                  nla_stopping *stop, int mf, int mos1, int mos2, double tolg)
{
    nla_evaluator ev;
    nla_local_spec spec = { NLA_LOCAL_TNEWTON, &ev, n, 1, 0, NULL, NULL, NULL, NULL, NULL, NULL, 0, 0, 0, 0, NULL, NULL, 0 };
    nla_lbfgs_params prm;
    nla_lbfgs_result res;
    char err[200];
    if (nla_dev_count() <= 0) { nla_stop_msg(stop, "nlopt_amd: no HIP device visible (this library has no CPU fallback)"); return NLOPT_FAILURE; }
    if (mos1 <= 0) mos1 = 1;                                  /* pnet.c:271-276 */
    if (mos2 <= 0) mos2 = 1;
    spec.mos = (mos1 - 1) + 2 * (mos2 - 1);
    spec.mf = mos2 > 1 ? nla_lbfgs_default_mf(n, mf, stop->maxeval) : 0;      /* pnet.c:590-594; no preconditioner, no history */
    nla_evaluator_resolve(&ev, opt, f, f_data);
    nla_local_params_from_stop(&prm, stop);
    prm.tolg = tolg;
    if (nla_local_run_batch(&spec, lb, ub, NULL, x, &prm, &res, stop, nla_exact_mode_for(opt, NULL, &ev),
                            ev.kind == NLA_EVAL_HOST ? stop->nevals_p : NULL, opt, err, sizeof err)) { nla_stop_msg(stop, "device engine: %s", err); return NLOPT_FAILURE; }
    *minf = res.f;
    if (ev.kind != NLA_EVAL_HOST) *stop->nevals_p += res.nevals;       /* host objective: counted call by call */
    return (nlopt_result) res.ret;                                       /* pnet.c:651-661: the kernel maps PNET's code (lb_result_of_iterm) */
}
