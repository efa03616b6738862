/* batch_driver.c — nlopt_amd_optimize_batch (include/nlopt_amd.h): many local searches of ONE optimiser in one call.
 *
 * The reference has no counterpart: a caller with many starts, or with many small fits of one shape, loops over nlopt_optimize.  Here
 * the loop is the batch dimension of the kernels that already serve MLSL's local phase — one workgroup (LD_LBFGS, LD_MMA) or one
 * wavefront (LN_COBYLA, LN_NELDERMEAD, LN_SBPLX) per search; LD_TNEWTON and its three variants (one workgroup) joined them — behind the same context a lone nlopt_optimize(LD_LBFGS | LD_MMA | LN_NELDERMEAD | LN_SBPLX) runs on with count = 1
 * (local_ctx.c: nla_local_batch_open / nla_local_ctx_run).  Those kernels pick their code path from the objective, n and the
 * parameters, never from the number of searches, which is what makes search i of a batch the lone run from x_i bit for bit.
 *
 * What this file adds: the checks (everything is refused before anything is touched), the direction of optimisation, the chunks —
 * at most `cap` searches per launch, cap from the free device memory — and, for a row-data objective (ABI 3, userobj.c), the first
 * data row of each chunk.
 *
 * Nonlinear constraints.  Served: NLOPT_LN_COBYLA on a user device objective (ABI 1, 2 or 3) when EVERY constraint entry is a bound device
 * block (usercon.c; ABI 1 or 2, one data block shared by all searches) and the constrained launcher (hip/cobyla_con.hip) serves
 * (n, mc = inequality values + 2 x equality values).  The context then runs every step as: the search kernel, the objective's kernel
 * for the waiting searches, one launch per block over the chunk's rows, the search kernel again (local_ctx.c).  Refused: LD_LBFGS /
 * LD_MMA with constraints, a constraint that is a host callback, a compiled-in or host objective with constraints, (n, mc) beyond the
 * launcher, a device layer without it.  Contract: search i is the lone nlopt_optimize(LN_COBYLA) of the same optimiser from x_i —
 * cobyla_host.c, which with no host twins bound evaluates single points through the same kernels. */
#include "nla_internal.h"
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define BATCH_FALLBACK_BUDGET ((size_t) 1 << 30)      /* a device layer that cannot say how much memory is free: chunks within 1 GiB */
#define BATCH_MAX_CHUNK (1 << 20)

nlopt_result nlopt_amd_optimize_batch(nlopt_opt opt, size_t count, double *x, double *minf, nlopt_result *results, int *numevals)
{
    nla_run_direction dir;
    nla_stopping stop;
    nla_evaluator ev;
    nla_mma_params mma;
    nla_lbfgs_params prm;
    nla_lbfgs_result *res = NULL;
    nla_local_batch B;
    nla_local_spec spec;
    nlopt_result ret = NLOPT_FAILURE;
    char err[200];
    double dummy;
    size_t first, per, budget, cap;
    unsigned n, i;
    int rc, on_device, total = 0, ncon = 0, mi = 0, me = 0;
    int64_t rows;
    nla_usercon **con = NULL;
    double *con_tol = NULL;

    if (!opt) return NLOPT_INVALID_ARGS;
    nla_unset_errmsg(opt);
    memset(&mma, 0, sizeof mma);
    memset(&B, 0, sizeof B);
    memset(&spec, 0, sizeof spec);
    n = opt->n;
    if (count == 0 || !x || !minf || !results) { nla_set_errmsg(opt, "nlopt_amd_optimize_batch: count == 0 or a NULL array"); return NLOPT_INVALID_ARGS; }
    if (count > (size_t) INT_MAX) { nla_set_errmsg(opt, "nlopt_amd_optimize_batch: count > INT_MAX"); return NLOPT_INVALID_ARGS; }
    if (!opt->f || n == 0) { nla_set_errmsg(opt, "nlopt_amd_optimize_batch: no objective set, or n == 0"); return NLOPT_INVALID_ARGS; }
    spec.alg = opt->algorithm == NLOPT_LD_LBFGS ? NLA_LOCAL_LBFGS : opt->algorithm == NLOPT_LD_MMA ? NLA_LOCAL_MMA : opt->algorithm == NLOPT_LN_COBYLA ? NLA_LOCAL_COBYLA :
               opt->algorithm == NLOPT_LN_NELDERMEAD ? NLA_LOCAL_NLDRMD : opt->algorithm == NLOPT_LN_SBPLX ? NLA_LOCAL_SBPLX :
               nla_is_tnewton(opt->algorithm) && nla_tnewton_has_launcher() ? NLA_LOCAL_TNEWTON : -1;
    if (spec.alg < 0) {
        nla_set_errmsg(opt, "nlopt_amd_optimize_batch serves NLOPT_LD_LBFGS, NLOPT_LD_MMA, NLOPT_LN_COBYLA, NLOPT_LN_NELDERMEAD and NLOPT_LN_SBPLX, not %s (and NLOPT_LD_TNEWTON with its three variants on a device layer that has their launcher)",
                       nlopt_algorithm_to_string(opt->algorithm));
        return NLOPT_INVALID_ARGS;
    }
    if (opt->m > 0 || opt->p > 0) {
        unsigned j;
        size_t vi = 0, ve = 0;
        if (opt->algorithm != NLOPT_LN_COBYLA) {
            nla_set_errmsg(opt, "nlopt_amd_optimize_batch: nonlinear constraints are served for NLOPT_LN_COBYLA only, not for %s", nlopt_algorithm_to_string(opt->algorithm));
            return NLOPT_INVALID_ARGS;
        }
        for (j = 0; j < opt->m + opt->p; ++j) {
            const nla_constraint *cj = j < opt->m ? opt->fc + j : opt->h + (j - opt->m);
            if (!nla_usercon_of(cj)) {
                nla_set_errmsg(opt, "nlopt_amd_optimize_batch: nonlinear constraints of a batch must be device blocks (nlopt_amd_add_*_device_mconstraint): %s constraint %u is a host callback",
                               j < opt->m ? "inequality" : "equality", j < opt->m ? j : j - opt->m);
                return NLOPT_INVALID_ARGS;
            }
            *(j < opt->m ? &vi : &ve) += cj->m;
        }
        if (!nla_userobj_is_adapter(opt->f)) {
            nla_set_errmsg(opt, "nlopt_amd_optimize_batch: nonlinear constraints are served with a user device objective (nlopt_amd_set_min/max_device_objective) only");
            return NLOPT_INVALID_ARGS;
        }
        if (!nla_cobyla_con_has_launcher()) {
            nla_set_errmsg(opt, "nlopt_amd_optimize_batch: this device layer has no LN_COBYLA launcher for nonlinear constraints");
            return NLOPT_INVALID_ARGS;
        }
        if (vi > 100000 || ve > 100000 || !nla_cobyla_con_serves((int) n, (int) (vi + 2 * ve))) {
            nla_set_errmsg(opt, "nlopt_amd_optimize_batch: no device LN_COBYLA launcher serves n = %u with %zu inequality and %zu equality values", n, vi, ve);
            return NLOPT_INVALID_ARGS;
        }
        ncon = (int) (opt->m + opt->p); mi = (int) vi; me = (int) ve;
    }
    if (opt->algorithm == NLOPT_LN_NELDERMEAD) {
        if (!nla_nldrmd_has_launcher()) { nla_set_errmsg(opt, "nlopt_amd_optimize_batch: this device layer has no LN_NELDERMEAD launcher"); return NLOPT_INVALID_ARGS; }
        if (n > NLA_NLDRMD_MAX_N || !nla_nldrmd_serves((int) n)) {
            nla_set_errmsg(opt, "nlopt_amd_optimize_batch: the device LN_NELDERMEAD launcher serves n <= %d, not n = %u", NLA_NLDRMD_MAX_N, n);
            return NLOPT_INVALID_ARGS;
        }
    }
    if (opt->algorithm == NLOPT_LN_SBPLX) {
        if (!nla_sbplx_has_launcher()) { nla_set_errmsg(opt, "nlopt_amd_optimize_batch: this device layer has no LN_SBPLX launcher"); return NLOPT_INVALID_ARGS; }
        if (n > NLA_SBPLX_MAX_N || !nla_sbplx_serves((int) n)) {
            nla_set_errmsg(opt, "nlopt_amd_optimize_batch: the device LN_SBPLX launcher serves n <= %d, not n = %u", NLA_SBPLX_MAX_N, n);
            return NLOPT_INVALID_ARGS;
        }
    }
    if (opt->comm) { nla_set_errmsg(opt, "nlopt_amd_optimize_batch: a communicator is set (nlopt_amd_set_comm): multi-rank batches are not served"); return NLOPT_INVALID_ARGS; }
    for (i = 0; i < n; ++i)
        if (opt->lb[i] == opt->ub[i]) {
            nla_set_errmsg(opt, "nlopt_amd_optimize_batch: lb[%u] == ub[%u]: the elimination of fixed coordinates is out of scope here (run such a box through nlopt_optimize)", i, i);
            return NLOPT_INVALID_ARGS;
        }
    for (first = 0; first < count; ++first)
        for (i = 0; i < n; ++i) {
            const double xi = x[first * n + i];
            if (opt->lb[i] > opt->ub[i] || xi < opt->lb[i] || xi > opt->ub[i]) {     /* (as the prologue of a lone run checks, optimize.c:546-552) */
                nla_set_errmsg(opt, "search %zu: bounds %u fail %g <= %g <= %g", first, i, opt->lb[i], xi, opt->ub[i]);
                return NLOPT_INVALID_ARGS;
            }
        }
    on_device = nlopt_amd_objective_id(opt->f) >= 0 || nla_userobj_is_adapter(opt->f);
    if (opt->algorithm == NLOPT_LN_COBYLA) {
        if (!on_device) { nla_set_errmsg(opt, "nlopt_amd_optimize_batch: LN_COBYLA is served for device objectives only (compiled-in or user-supplied)"); return NLOPT_INVALID_ARGS; }
        if (!nla_cobyla_device_serves(nla_userobj_is_adapter(opt->f) ? NLA_EVAL_USER : NLA_EVAL_DEVICE, (int) n)) {
            nla_set_errmsg(opt, "nlopt_amd_optimize_batch: no device LN_COBYLA launcher serves n = %u", n);
            return NLOPT_INVALID_ARGS;
        }
    }
    rows = nla_userobj_is_adapter(opt->f) ? nla_userobj_data_rows(opt->userobj) : -1;
    if (rows >= 0 && (int64_t) count > rows) {
        nla_set_errmsg(opt, "nlopt_amd_optimize_batch: search i reads data row i: %zu searches, %lld rows set (nlopt_amd_set_device_objective_row_data)", count, (long long) rows);
        return NLOPT_INVALID_ARGS;
    }
    if (opt->algorithm == NLOPT_LD_MMA && (rc = nla_mma_read_params(opt, &mma))) return (nlopt_result) rc;
    if (nla_dev_count() <= 0) { nla_set_errmsg(opt, "nlopt_amd: no HIP device visible (this library has no CPU fallback)"); return NLOPT_FAILURE; }

    if (ncon) {                                          /* the blocks and their tolerances in the reference's order (cobyla.c:242-251) */
        unsigned j, k, t = 0;
        con = (nla_usercon **) malloc(sizeof *con * (size_t) ncon);
        con_tol = (double *) malloc(sizeof(double) * (size_t) (mi + me));
        if (!con || !con_tol) { free(con); free(con_tol); nla_set_errmsg(opt, "out of memory"); return NLOPT_OUT_OF_MEMORY; }
        for (j = 0; j < opt->m + opt->p; ++j) {
            const nla_constraint *cj = j < opt->m ? opt->fc + j : opt->h + (j - opt->m);
            con[j] = nla_usercon_of(cj);
            for (k = 0; k < cj->m; ++k) con_tol[t++] = cj->tol ? cj->tol[k] : 0.;
        }
    }

    /* from here on the run: what nlopt_optimize does in front of a lone search */
    nlopt_set_force_stop(opt, 0);
    opt->force_stop_child = NULL;
    nla_direction_enter(opt, on_device, &dir);
    if ((ret = nla_setup_run(opt, x, &dummy, &stop)) != NLOPT_SUCCESS) goto leave;
    ret = NLOPT_FAILURE;
    nla_evaluator_resolve(&ev, opt, opt->f, opt->f_data);
    nla_local_params_from_stop(&prm, &stop);
    spec.ev = &ev; spec.n = (int) n; spec.mma = &mma;
    opt->batch_con_launches = 0;
    spec.con = con; spec.ncon = ncon; spec.ncon_eq = ncon ? (int) opt->p : 0; spec.mi = mi; spec.me = me; spec.con_tol = con_tol;
    spec.con_launches = &opt->batch_con_launches;
    if (nla_is_tnewton(opt->algorithm)) {                /* as nla_tnewton_minimize sets a lone run up */
        spec.mos = (int) opt->algorithm - (int) NLOPT_LD_TNEWTON;
        prm.tolg = nlopt_get_param(opt, "tolg", 0.);
        spec.mf = spec.mos >= 2 ? nla_lbfgs_default_mf((int) n, (int) opt->vector_storage, stop.maxeval) : 0;
    }
    if (opt->algorithm == NLOPT_LD_LBFGS) { prm.tolg = nlopt_get_param(opt, "tolg", 0.); spec.mf = nla_lbfgs_default_mf((int) n, (int) opt->vector_storage, stop.maxeval); }

    /* the chunk: what fits half of the free memory (the other half is the caller's, and the allocator's slack) */
    per = nla_local_ctx_bytes_per_search_con(spec.alg, &ev, (int) n, spec.mf, mi, me);
    budget = nla_dev_mem_free_bytes ? nla_dev_mem_free_bytes() / 2 : 0;
    if (budget == 0) budget = BATCH_FALLBACK_BUDGET;
    cap = budget / (per ? per : 1);
    if (nlopt_get_param(opt, "amd_batch_chunk", 0.) >= 1.) cap = (size_t) nlopt_get_param(opt, "amd_batch_chunk", 0.);
    if (cap > BATCH_MAX_CHUNK) cap = BATCH_MAX_CHUNK;
    if (cap > count) cap = count;
    if (cap < 1) cap = 1;

    res = (nla_lbfgs_result *) malloc(sizeof *res * cap);
    if (!res) { nla_set_errmsg(opt, "out of memory"); ret = NLOPT_OUT_OF_MEMORY; goto leave; }
    spec.cap = (int) cap;
    if (nla_local_batch_open(&B, &spec, opt->lb, opt->ub, opt->dx, &stop, nla_exact_mode_for(opt, NULL, &ev), err, sizeof err)) {
        nla_set_errmsg(opt, "device engine: %s", err);
        goto leave;
    }
    nla_local_ctx_set_stats(B.c, &opt->stats);
    nla_local_ctx_set_cobyla_min_batch(B.c, 1);          /* never the host algorithm: a search's bits must not depend on the batch size */
    /* the waiting list of a user kernel's step: the host loop unless "amd_batch_host_list" = 0 asks for the device-built one — measured
     * (profiles/r11_batch_fit.txt) the device list did not win at the batch sizes tried, so the default stays where MLSL's path is */
    opt->local_list_launches = 0;
    nla_local_ctx_set_device_list(B.c, nlopt_get_param(opt, "amd_batch_host_list", 1.) == 0., &opt->local_list_launches);

    for (first = 0; first < count; first += cap) {
        const size_t k = count - first < cap ? count - first : cap;
        size_t j;
        nla_local_ctx_set_row0(B.c, (int64_t) first);
        if (nla_local_batch_upload(&B, (int) k, x + first * n, err, sizeof err)) { nla_set_errmsg(opt, "device engine: %s", err); goto close; }
        if ((rc = nla_local_ctx_run(B.c, (int) k, &prm, res, &stop, ev.kind == NLA_EVAL_HOST ? stop.nevals_p : NULL))) {
            nla_set_errmsg(opt, "device engine: local-search batch failed: %s", nla_dev_error_string(rc));
            goto close;
        }
        if (nla_local_batch_download(&B, (int) k, x + first * n, err, sizeof err)) { nla_set_errmsg(opt, "device engine: %s", err); goto close; }
        for (j = 0; j < k; ++j) {
            minf[first + j] = dir.maximize ? -res[j].f : res[j].f;
            results[first + j] = (nlopt_result) res[j].ret;
            if (numevals) numevals[first + j] = res[j].nevals;
            total += res[j].nevals;
        }
    }
    opt->numevals = total;                               /* (a host objective was counted call by call meanwhile: the same sum) */
    ret = nla_stop_forced(&stop) ? NLOPT_FORCED_STOP : NLOPT_SUCCESS;
    if (ret == NLOPT_SUCCESS && nla_stop_time(&stop))
        for (first = 0; first < count; ++first) if (results[first] == NLOPT_MAXTIME_REACHED) { ret = NLOPT_MAXTIME_REACHED; break; }
close:
    nla_local_batch_close(&B);
leave:
    free(res); free(con); free(con_tol);
    nla_direction_leave(opt, &dir);
    return ret;
}

uint64_t nlopt_amd_local_list_launches(const nlopt_opt opt) { return opt ? opt->local_list_launches : 0; }
uint64_t nlopt_amd_batch_constraint_launches(const nlopt_opt opt) { return opt ? opt->batch_con_launches : 0; }
