/* crs_entry.c — CRS2_LM at the API level: the reference-shaped entry point and the stepwise sessions of nlopt_amd.h.  Both decide the
 * run's mode (windows or conservative passes, sharded or not), create the HIP engine (crs_engine.h) and hand it to the driver
 * (crs_driver.c). */
#include "crs_engine.h"

static nlopt_result crs_open_common(nlopt_opt opt, int n, nlopt_func f, void *f_data, const double *lb, const double *ub, const double *x,
                                    nla_stopping *stop, int population, nla_crs_problem *pb, nla_crs_hip_engine **eout)
{
    int64_t N = population ? (int64_t) population : 10 * ((int64_t) n + 1);     /* crs.c:172-179 */
    nla_crs_engine_config cfg = { 0 };
    *eout = NULL;
    if (N < n + 1) {                                                            /* crs.c:180-184 */
        nla_stop_msg(stop, "population %d should be >= dimension + 1 = %d", (int) N, n + 1);
        return NLOPT_INVALID_ARGS;
    }
    memset(pb, 0, sizeof *pb);
    pb->forward = n >= NLA_CRS_FORWARD_MIN_N;
    pb->n = n; pb->N = N; pb->lb = lb; pb->ub = ub; pb->f = f; pb->f_data = f_data; pb->stop = stop;
    {
        nla_evaluator ev;
        nla_evaluator_resolve(&ev, opt, f, f_data);
        pb->obj = ev.kind == NLA_EVAL_DEVICE ? ev.obj : (ev.kind == NLA_EVAL_USER ? -2 : -1);
        cfg.user = ev.user; cfg.sign = ev.sign;
    }
    if (opt) {
        pb->trace = opt->trace; pb->trace_cap = opt->trace_cap; pb->trace_len = &opt->trace_len;
        pb->stats = &opt->stats;
        pb->max_spec = (int) nlopt_get_param(opt, "amd_max_spec", 0);
        pb->window_factor = nlopt_get_param(opt, "amd_window_factor", 0);
        /* device-resolved windows (hip/crs_chain.hip, the chain advanced by the resolver wavefront) at every dimension.  Measured on the
         * MI355X, N = 1e5 (profiles/r05_staged_ab.txt; conservative passes -> windows -> windows of 256 slots): n = 64 1.26 -> 1.44 -> 1.56 M
         * evals/s, n = 128 1.07 -> 1.32 -> 1.39 M, n = 256 0.75 -> 1.03 -> 1.08 M, n = 512 (round 4) 445 -> 606 k */
        pb->forward = nlopt_get_param(opt, "amd_forward", n >= NLA_CRS_FORWARD_MIN_N ? 1 : 0) != 0;
        pb->forward = nla_dbg_int("NLA_CRS_FORWARD", pb->forward);                 /* A/B switch for the bench */
        if (nlopt_get_param(opt, "amd_host_eval", 0) != 0) pb->obj = -1;   /* force the host-callback path */
    }
    if (nla_dev_count() <= 0) {
        nla_stop_msg(stop, "nlopt_amd: no HIP device visible (this library has no CPU fallback)");
        nla_comm_agree_ready(opt ? opt->comm : NULL, 0);
        return NLOPT_FAILURE;
    }
    {
        /* several ranks and a compiled-in objective: the population is sharded by coordinate and the window runs as conservative
         * passes on every rank's slice ("amd_shard" = 0: every rank keeps the whole population — replicas of the one chain) */
        nlopt_amd_comm *comm = opt ? opt->comm : NULL;
        const int shard = comm && nla_crs_can_shard(n, nlopt_amd_comm_world(comm)) && pb->obj >= 0 &&
                          (!opt || nlopt_get_param(opt, "amd_shard", 1) != 0);
        /* ... or, where the coordinates can be dealt in whole 128-byte lines over at most 8 ranks, as device-resolved windows whose slices
         * cross between the ranks' kernels through peer-mapped memory ("amd_shard_windows" = 0: the conservative passes;
         * "amd_cu_share" = k: k ranks share one device — each rank's windows run on its k-th of the compute units) */
        const int windows = shard && pb->forward && pb->max_spec != 1 /* (a window of one slot: the driver runs conservative passes) */ &&
                            nla_crs_can_shard_windows(n, nlopt_amd_comm_world(comm)) &&
                            (!opt || nlopt_get_param(opt, "amd_shard_windows", 1) != 0);
        const int cu_parts = opt ? (int) nlopt_get_param(opt, "amd_cu_share", 0) : 0;
        if (shard) { pb->comm = comm; if (!windows) pb->forward = 0; }
        cfg.n = n; cfg.N = N; cfg.lb = lb; cfg.ub = ub; cfg.obj = pb->obj; cfg.forward = pb->forward; cfg.comm = comm; cfg.stats = pb->stats;
        cfg.shard = windows ? 2 : shard; cfg.cu_parts = windows || !comm ? cu_parts : 0;
        *eout = nla_crs_hip_engine_create(&cfg);
        if (windows) {
            /* all ranks run windows, or all fall back to the conservative passes (a rank that could not map a peer's buffers, an
             * allocation that failed): the same decision everywhere */
            const int all = nla_comm_agree_ready(comm, *eout != NULL);
            if (!all) {
                if (*eout) nla_crs_hip_engine_destroy(*eout, 0);
                pb->forward = 0;
                cfg.forward = 0; cfg.shard = 1; cfg.cu_parts = 0;
                *eout = nla_crs_hip_engine_create(&cfg);
            }
        }
    }
    /* several ranks: all of them go on, or none (a rank that could not set up would leave the others in the first all-gather) */
    if (opt && nlopt_amd_comm_world(opt->comm) > 1) {
        const int all = nla_comm_agree_same(opt->comm, *eout != NULL, nla_problem_fingerprint(NLOPT_GN_CRS2_LM, n, (int) N, pb->obj, lb, ub, x, stop) + nla_params_fingerprint(opt));
        if (all <= 0 && *eout) {
            nla_crs_hip_engine_destroy(*eout, 0); *eout = NULL;
            if (all < 0) { nla_stop_msg(stop, NLA_MSG_RANKS_DIFFER); return NLOPT_INVALID_ARGS; }
            nla_stop_msg(stop, "nlopt_amd: another rank could not set up its device engine");
            return NLOPT_FAILURE;
        }
    }
    if (!*eout) {
        nla_stop_msg(stop, "nlopt_amd: could not create the device engine (out of device memory?)");
        return NLOPT_OUT_OF_MEMORY;
    }
    return NLOPT_SUCCESS;
}

/* reference-shaped entry point: crs_minimize(n, f, f_data, lb, ub, x, minf, stop, population, lds=0)
 * (src/algs/crs/crs.h:34-40; called from the dispatcher as at src/api/optimize.c:744-747) */
nlopt_result nla_crs_minimize(nlopt_opt opt, int n, nlopt_func f, void *f_data, const double *lb, const double *ub,
                              double *x, double *minf, nla_stopping *stop, int population)
{
    nla_crs_problem pb;
    nla_crs_hip_engine *e;
    nlopt_result ret;
    uint64_t words = 0;
    ret = crs_open_common(opt, n, f, f_data, lb, ub, x, stop, population, &pb, &e);
    if (ret != NLOPT_SUCCESS) return ret;
    ret = nla_crs_run(&nla_crs_hip_ops, e, &pb, x, minf, &words);
    if (pb.stats) pb.stats->mt_words = words;
    nla_crs_hip_engine_destroy(e, words);
    return ret;
}

/* ---- stepwise sessions (nlopt_amd.h): the same run, paused between speculation rounds ---------- */
struct nlopt_amd_crs_session {
    nlopt_opt opt;
    nla_stopping stop;
    nla_crs_problem pb;
    nla_crs_hip_engine *e;
    nla_crs_session *S;
    nlopt_result ret;
};

nlopt_result nla_setup_run(nlopt_opt opt, double *x, double *minf, nla_stopping *stop);

nlopt_amd_crs_session *nlopt_amd_crs_open(nlopt_opt opt, double *x, double *minf, nlopt_result *ret_out)
{
    nlopt_amd_crs_session *h;
    nlopt_result ret;
    int pop;
    nla_unset_errmsg(opt);
    if (!opt || opt->algorithm != NLOPT_GN_CRS2_LM || opt->maximize) { if (ret_out) *ret_out = NLOPT_INVALID_ARGS; return NULL; }
    h = (nlopt_amd_crs_session *) calloc(1, sizeof *h);
    if (!h) { if (ret_out) *ret_out = NLOPT_OUT_OF_MEMORY; return NULL; }
    h->opt = opt;
    nlopt_set_force_stop(opt, 0);
    ret = nla_setup_run(opt, x, minf, &h->stop);
    if (ret == NLOPT_SUCCESS) {
        pop = opt->stochastic_population > 0 ? (int) opt->stochastic_population
                                             : (nla_stochastic_population > 0 ? nla_stochastic_population : 0);
        ret = crs_open_common(opt, (int) opt->n, opt->f, opt->f_data, opt->lb, opt->ub, x, &h->stop, pop, &h->pb, &h->e);
    }
    if (ret != NLOPT_SUCCESS) { if (ret_out) *ret_out = ret; free(h); return NULL; }
    h->S = nla_crs_begin(&nla_crs_hip_ops, h->e, &h->pb, x, minf, &ret);
    h->ret = ret;
    if (ret_out) *ret_out = ret;
    if (!h->S) { nla_crs_hip_engine_destroy(h->e, 0); free(h); return NULL; }
    return h;
}

nlopt_result nlopt_amd_crs_step(nlopt_amd_crs_session *h, long eval_budget)
{
    if (!h || !h->S) return NLOPT_INVALID_ARGS;
    if (h->ret == NLOPT_SUCCESS) h->ret = nla_crs_advance(h->S, (int64_t) eval_budget);
    return h->ret;
}

nlopt_result nlopt_amd_crs_close(nlopt_amd_crs_session *h)
{
    nlopt_result ret;
    uint64_t words = 0;
    if (!h) return NLOPT_INVALID_ARGS;
    ret = nla_crs_end(h->S, &words);
    if (h->pb.stats) h->pb.stats->mt_words = words;
    nla_crs_hip_engine_destroy(h->e, words);
    free(h);
    return ret;
}
