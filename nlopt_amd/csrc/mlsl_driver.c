#define _GNU_SOURCE            /* qsort_r */
/* mlsl_driver.c — Multi-Level Single-Linkage behind the reference's entry point
 *   mlsl_minimize(n, f, f_data, lb, ub, x, minf, stop, local_opt, Nsamples, lds)   (mlsl.h:34-41),
 * host side: the point / local-minimum bookkeeping of mlsl.c:251-438 (ordered by f, the trees'
 * tie rule kept), stop tests in the reference's order, stream accounting; device side through
 * the C-ABI launchers of include/nlopt_amd.h:
 *
 *   sampling phase (mlsl.c:349-374)   the N samples of an iteration are generated from the stream
 *       and evaluated in one launch; all pair distances new x (old + new) and new x minima in one
 *       tiled kernel (bit-identical distances); closest_pt_d / closest_lm_d by masked min kernels.
 *       The reference interleaves these per sample; the values it reads later (only in the local
 *       phase) are mins over the same pair sets, so batching changes nothing.
 *   local phase (mlsl.c:380-428)      the walk over the best ceil(gamma |pts|) points is serial in the
 *       reference because a new minimum can disqualify later candidates (closest_lm_d only ever
 *       decreases).  Here the next batch of currently-potential candidates is minimised
 *       concurrently — one workgroup each in the batched L-BFGS kernel — and committed in walk
 *       order; a candidate that an earlier commit of the same batch disqualified is dropped
 *       (its start point stays un-minimised, exactly as if it had never been started).
 *   multi-GPU (nlopt_amd_set_comm)    every rank runs this same driver on the same stream (sampling and
 *       bookkeeping are replicated, they are cheap); the candidates of a batch are dealt round-robin over
 *       the ranks — candidate c is minimised by rank c mod world — and the minimisers + their results
 *       are ALL-GATHERED (SURVEY.md §8e "all-gather of local minima"), after which every rank commits
 *       the whole batch in walk order.  world x BATCH_MAX searches are in flight per batch.
 *
 * Objectives: compiled-in and user-supplied device objectives run batched as described; an ordinary host callback
 * (nlopt_func) is served with the reference's contract — f is called on the caller's thread, one point at a time, in the
 * reference's order (samples in order with the stop tests between them, mlsl.c:360-366; then one local search after the
 * other, mlsl.c:404) — while sampling, distances and every vector operation of the local searches stay on the device.
 *
 * Provided: local optimisers NLOPT_LD_LBFGS and NLOPT_LD_MMA (the GD_MLSL default); pseudo-random sampling (the non-LDS
 * variants, and the LDS variants for n > 1111 where the reference's Sobol generator is NULL — sobolseq.c:143
 * — and mlsl.c:355-359 falls back to nlopt_urand) and Sobol sampling (LDS variants, n <= 1111; points by
 * index, sobol.c; no MT words are drawn in that mode).
 */
#include "nla_internal.h"
#include "nla_switches.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#define NLA_MLSL_SEG_REGENS 64          /* segment length (in regenerations of 624 words) of an MLSL run's MT19937 device stream */

#define K2PI (6.2831853071795864769252867665590057683943388)
#define MLSL_SIGMA 2.
#define MLSL_GAMMA 0.3
#define BATCH_MAX 320                  /* local searches in flight per rank (one workgroup each) */

static double gam(int n) { double z = n / 2; return sqrt(pow(K2PI * z, 1.0 / n) * z) * exp(-0.5); }   /* mlsl.c:227-237 */

/* the objective as MLSL's local optimiser sees it (fcount, mlsl.c:246-251): every call counted where the caller can see it */
typedef struct { nlopt_func f; void *f_data; double sign; int *nevals_p; } mlsl_count_wrap;

/* who runs the local searches of a run — decided once, by mlsl_choose_local */
typedef enum {
    MLSL_HOST_SEARCH,               /* LN_COBYLA as a host algorithm (cobyla_host.c), one search at a time on the caller's thread */
    MLSL_DEV_COBYLA,                /* LN_COBYLA batched on the device */
    MLSL_LBFGS, MLSL_MMA            /* the batched device kernels (with a host callback: one search at a time, f on the caller's thread) */
} mlsl_local;

/* the state of one run: what every phase below reads, and everything the run allocates (mfree) */
typedef struct {
    /* the caller's */
    nlopt_opt opt, local_opt;
    nlopt_func f; void *f_data;     /* host evaluations (a maximisation left unflipped by the dispatcher: the flipped one, mlsl_signed_f) */
    nla_stopping *stop;
    /* several ranks: the clock and the force_stop flag are decided by all ranks together at the start of every phase (comm.c);
     * sp is what those two tests look at until the next agreement (mlsl_agree) */
    const nla_stopping *sp; nla_stopping agreed_view; int agreed_force;
    nla_stopping lstop;             /* what a local search observes of the caller's stopping state */
    nla_lbfgs_params prm; int loc_maxeval;
    nla_mma_params mma;
    mlsl_local local;
    int host;                       /* f is called on the caller's thread: a host callback, or the host search */
    int batch, bmax;                /* searches in flight per rank / over all ranks */
    double R_prefactor;
    nlopt_result ret;
    int search_failed;              /* a local search returned an error: the result is the best point known BEFORE the iteration (the reference's goto done) */
    double best_f; size_t best_row; int best_is_lm;
    /* the host search: the local optimiser's own objective while this run has its wrapper installed in it, and the wrappers' data */
    int lo_installed; nlopt_func lo_f; void *lo_fdata;
    mlsl_count_wrap cw, sw;
    /* per-batch arrays */
    nla_lbfgs_result *res, *res_mine;   /* all candidates' results by gathered row (bmax) / this rank's (BATCH_MAX) */
    size_t *cand;                   /* bmax: positions in `ord` of the batch's candidates */
    double *Fnew;                   /* pinned, N: the samples' values come back every iteration */
    double *cob_x;                  /* pinned, n: the host search's point */
    int prefetch_due, ahead_due;    /* to go out in front of the next launch of local searches (mlsl_prefetch_now) */

    int n, ld, obj, N;
    nla_evaluator ev;
    double *h_rows;                 /* host objective: the iteration's samples, pinned (N x ld) */
    void *rs;                       /* the generator's stream: st itself, or (prefetch) a second one */
    void *ev_samples;               /* recorded behind the copy of the samples' values (the distance pass is enqueued behind it) */
    int prefetch; uint64_t prefetched_at;   /* device objectives: the next iteration's sample words generated beside the local phase; stream position they were generated for */
    void *st;
    nla_mtstream *mts;
    uint64_t words_used;
    /* points: row id = insertion order */
    size_t npts, cap;
    double *F, *cpd, *cld;          /* host */
    int32_t *minimized;
    size_t *ord;                    /* row ids sorted by f, equal keys newest first (redblack.c:120) */
    int ord_has_nan;                /* a NaN key went in: from then on rows are inserted one by one (ord_insert_run) */
    size_t nlms, lcap;
    double *LF; size_t *lord;
    double *d_lb, *d_ub, *d_P, *d_F, *d_cpd, *d_LM, *d_LF, *d_D, *d_tmp;
    double *d_LX;                   /* gathered minimisers of a batch: world x per rows of ld */
    nlopt_amd_comm *comm; int world, rank;
    int32_t *d_min;
    uint32_t *d_words;
    double *d_dx;                         /* LD_MMA local optimiser: the initial step on the device, or NULL */
    uint32_t *d_V; uint32_t sobol_next;   /* LDS mode: direction table on the device, index of the next point (1-based) */
    size_t dcap;                    /* doubles in d_D */
    nla_local_ctx *lb;
    double *h_D;                    /* pinned: one row of npts distances (the rerun of a single search) */
    size_t hcap;
    double *h_S, *d_S;              /* bmax x bmax: distance between minimiser c' and start point c of a batch — all the commit walk reads of the batch's matrix */
    double *h_lfall, *d_lfall;      /* bmax: f of the accepted minima by gathered row, +inf for the others (the device-side pts_update_newlm) */
    double *lf_cand;                /* the same by CANDIDATE (what the commit walk's inner loop reads: no index arithmetic per question) */
    int64_t *h_gi, *d_gi;           /* bmax: gathered row of candidate c */
    double *h_gather; size_t gcap;  /* several ranks: world x count doubles for the element-wise min of the distance minima */
    /* per-batch lists, pinned host side + device side: [idx of all candidates: bmax][idx of this rank's: BATCH_MAX]
     * [gathered-row index of the accepted minima: bmax] as int64, then the accepted minima's f (bmax doubles); flags: bmax int32 */
    int64_t *h_idx, *d_idx;
    double *h_lf;
    int32_t *h_flags, *d_flags;
    /* THE NEXT ITERATION'S SAMPLING PHASE, AHEAD (round 5; one rank, compiled-in objective): nothing of a sampling phase but the distances to the
     * minima of the local phase before it depends on that local phase — not the sample points (the local optimisers draw no random
     * numbers), not their values, not their distances to the points and to the minima known so far.  All of it is enqueued on the
     * generator's background stream right in front of the local searches' launch (mlsl_enqueue_ahead) and runs beside it: the searches
     * are bound by memory latency on a quarter of the chip's wavefront slots, the distance pass by fp64 arithmetic.  The results wait in
     * buffers of their own (closest-point minima in d_cpd2 / h_cpd2, closest-minimum distances in h_cld2) and are merged by `min` —
     * which is what both updates are (mlsl.c:155-194) — when the iteration they belong to starts. */
    int ahead, ahead_valid;
    size_t ahead_old, ahead_nlms;    /* rows old .. old + N - 1 were sampled for a point set of `old` rows; minima 0 .. ahead_nlms - 1 are accounted for */
    uint64_t ahead_words; uint32_t ahead_sobol;
    void *ev_ahead;
    double *Fnew2, *h_cld2;          /* pinned, N each */
    double *d_D2; size_t dcap2;
    double *d_cpd2, *h_cpd2, *h_inf, *d_cld2; size_t cap2;
    /* ... and it STARTS when half of the searches it runs beside have ended (nla_k_gate on the searches' counter of finished ones): a
     * launch lasts as long as its longest search (2.2 - 6.0 ms at config 4, 3.7 on average), and whatever else the device works on
     * slows the searches by a quarter while it runs — on other compute units too (CU-masked streams: same loss), so no question of issue
     * slots or LDS — behind the gate that is the launch's thinning second half, not all of it (config 4: 9.7 -> 9.4 ms per iteration) */
    const int32_t *gate_counter; int32_t gate_from, gate_need;
    nlopt_amd_stats *stats;
    int32_t *h_gate_gave_up; int gate_off;      /* pinned word a gate sets when it times out: no more gates in this run (nlopt_amd_stats.mlsl_gate_timeouts) */
    char err[200];
} mlsl_dev;

#ifndef NLA_MLSL_GATE_PCT
#define NLA_MLSL_GATE_PCT 50        /* the sampling phase enqueued ahead starts when this share of the batch's searches have ended (0: at once) */
#endif
#define MFAIL(d, ...) do { snprintf((d)->err, sizeof (d)->err, __VA_ARGS__); return -1; } while (0)

/* the one teardown: everything the run allocated, and the local optimiser's own objective put back (the host search's wrapper and
 * its data live in the caller's frame) */
static void mfree(mlsl_dev *d)
{
    if (d->lo_installed) { d->local_opt->f = d->lo_f; d->local_opt->f_data = d->lo_fdata; d->lo_installed = 0; }
    nla_host_free(d->cob_x);
    if (d->st) nla_stream_sync(d->st);
    if (d->rs) nla_stream_sync(d->rs);
    if (d->mts) { nla_mtstream_finish(d->mts, d->words_used); nla_mtstream_destroy(d->mts); }
    nla_local_ctx_destroy(d->lb);
    free(d->F); nla_host_free(d->cpd); nla_host_free(d->cld); nla_host_free(d->minimized); free(d->ord); free(d->LF); free(d->lord);
    nla_dev_free(d->d_lb); nla_dev_free(d->d_ub); nla_dev_free(d->d_P); nla_dev_free(d->d_F); nla_dev_free(d->d_cpd);
    nla_dev_free(d->d_LM); nla_dev_free(d->d_LF); nla_dev_free(d->d_D); nla_dev_free(d->d_tmp); nla_dev_free(d->d_min);
    nla_dev_free(d->d_words); nla_dev_free(d->d_LX); nla_dev_free(d->d_V); nla_dev_free(d->d_dx);
    nla_host_free(d->h_rows);
    free(d->h_gather);
    nla_host_free(d->h_D); nla_host_free(d->h_idx); nla_host_free(d->h_lf); nla_host_free(d->h_flags);
    nla_host_free(d->h_S); nla_host_free(d->h_lfall); nla_host_free(d->h_gi); free(d->lf_cand);
    nla_dev_free(d->d_idx); nla_dev_free(d->d_flags); nla_dev_free(d->d_S); nla_dev_free(d->d_lfall); nla_dev_free(d->d_gi);
    nla_event_destroy(d->ev_samples); nla_event_destroy(d->ev_ahead);
    nla_host_free(d->h_gate_gave_up); nla_host_free(d->Fnew2); nla_host_free(d->h_cld2); nla_host_free(d->h_cpd2); nla_host_free(d->h_inf);
    nla_dev_free(d->d_D2); nla_dev_free(d->d_cpd2); nla_dev_free(d->d_cld2);
    if (d->rs && d->rs != d->st) nla_stream_destroy(d->rs);
    if (d->st) nla_stream_destroy(d->st);
    nla_host_free(d->Fnew); free(d->res); free(d->res_mine); free(d->cand);
}

/* host arrays that travel to / from the device every iteration live in PINNED memory: a copy from pageable memory is staged by the
 * runtime and was seen to hold the main stream's work back until the generator's stream had drained (the sample prefetch did not
 * overlap anything, profiles/r04_mlsl_prefetch_timeline.txt) */
static void *pinned_regrow(void *old, size_t old_bytes, size_t new_bytes)
{
    void *p = nla_host_malloc(new_bytes);
    if (p && old && old_bytes) memcpy(p, old, old_bytes);
    if (p) nla_host_free(old);
    return p;
}
static int grow_pts(mlsl_dev *d, size_t need)
{
    size_t ncap = d->cap ? d->cap : 1024;
    double *nP, *nF, *nC;
    int32_t *nM;
    if (need <= d->cap) return 0;
    if (!d->cap) {
        /* the first allocation holds 16 iterations' samples (within 2 GiB of rows; 524 MB at config 4 of 288 GB): growing costs a
         * round of allocations, a copy of the whole point set and frees that wait for the device — 0.9 ms in the middle of one of
         * the first iterations each time the set doubled (profiles/r05_mlsl_timeline.txt) */
        const size_t want = 16 * (size_t) d->N + 1, budget = ((size_t) 2 << 30) / (sizeof(double) * (size_t) d->ld);
        const size_t first = want < budget ? want : budget;
        if (first > ncap) ncap = first;          /* exactly the budgeted rows: rounding up to a power of two could double the 2 GiB (advisor, round 5) */
    }
    while (ncap < need) ncap *= 2;
    d->F = (double *) realloc(d->F, sizeof(double) * ncap);
    {
        double *c1 = (double *) pinned_regrow(d->cpd, sizeof(double) * d->cap, sizeof(double) * ncap);
        double *c2 = (double *) pinned_regrow(d->cld, sizeof(double) * d->cap, sizeof(double) * ncap);
        int32_t *m1 = (int32_t *) pinned_regrow(d->minimized, sizeof(int32_t) * d->cap, sizeof(int32_t) * ncap);
        if (c1) d->cpd = c1;
        if (c2) d->cld = c2;
        if (m1) d->minimized = m1;
        if (!c1 || !c2 || !m1) MFAIL(d, "out of pinned memory growing the point set");
    }
    /* (with the point set, not in the local phase when a row of distances first exceeds it: freeing pinned memory waits for the device —
     * 0.53 ms + 0.04 ms for the new block between the searches' results and the commit walk, in every iteration that crossed the old
     * size; host-side API trace of config 4, round 5) */
    nla_host_free(d->h_D);
    d->h_D = (double *) nla_host_malloc(sizeof(double) * ncap);
    d->hcap = d->h_D ? ncap : 0;
    if (!d->h_D) MFAIL(d, "out of pinned memory growing the point set");
    d->ord = (size_t *) realloc(d->ord, sizeof(size_t) * ncap);
    nP = (double *) nla_dev_malloc(sizeof(double) * ncap * (size_t) d->ld);
    nF = (double *) nla_dev_malloc(sizeof(double) * ncap);
    nC = (double *) nla_dev_malloc(sizeof(double) * ncap);
    nM = (int32_t *) nla_dev_malloc(sizeof(int32_t) * ncap);
    if (!d->F || !d->cpd || !d->cld || !d->minimized || !d->ord || !nP || !nF || !nC || !nM) {
        nla_dev_free(nP); nla_dev_free(nF); nla_dev_free(nC); nla_dev_free(nM);
        MFAIL(d, "out of memory growing the point set");
    }
    if (d->npts && (nla_memcpy_d2d(nP, d->d_P, sizeof(double) * d->npts * (size_t) d->ld, d->st) ||
                    nla_memcpy_d2d(nF, d->d_F, sizeof(double) * d->npts, d->st) || nla_stream_sync(d->st))) {
        nla_dev_free(nP); nla_dev_free(nF); nla_dev_free(nC); nla_dev_free(nM);
        MFAIL(d, "copying the point set failed");
    }
    nla_dev_free(d->d_P); nla_dev_free(d->d_F); nla_dev_free(d->d_cpd); nla_dev_free(d->d_min);
    d->d_P = nP; d->d_F = nF; d->d_cpd = nC; d->d_min = nM;
    d->cap = ncap;
    return 0;
}

static int grow_lms(mlsl_dev *d, size_t need)
{
    size_t ncap = d->lcap ? d->lcap : 256;
    double *nL, *nF;
    if (need <= d->lcap) return 0;
    if (!d->lcap) {           /* (as the point set: room for 8 iterations' worth of minima from the start, within 1 GiB) */
        const size_t want = 8 * (size_t) d->N, budget = ((size_t) 1 << 30) / (sizeof(double) * (size_t) d->ld);
        const size_t first = want < budget ? want : budget;
        if (first > ncap) ncap = first;
    }
    while (ncap < need) ncap *= 2;
    d->LF = (double *) realloc(d->LF, sizeof(double) * ncap);
    d->lord = (size_t *) realloc(d->lord, sizeof(size_t) * ncap);
    nL = (double *) nla_dev_malloc(sizeof(double) * ncap * (size_t) d->ld);
    nF = (double *) nla_dev_malloc(sizeof(double) * ncap);
    if (!d->LF || !d->lord || !nL || !nF) { nla_dev_free(nL); nla_dev_free(nF); MFAIL(d, "out of memory growing the local-minimum set"); }
    if (d->nlms && (nla_memcpy_d2d(nL, d->d_LM, sizeof(double) * d->nlms * (size_t) d->ld, d->st) ||
                    nla_memcpy_d2d(nF, d->d_LF, sizeof(double) * d->nlms, d->st) || nla_stream_sync(d->st))) {
        nla_dev_free(nL); nla_dev_free(nF);
        MFAIL(d, "copying the local-minimum set failed");
    }
    nla_dev_free(d->d_LM); nla_dev_free(d->d_LF);
    d->d_LM = nL; d->d_LF = nF; d->lcap = ncap;
    return 0;
}

/* The distance scratch grows with the point set — N x npts doubles per sampling phase, npts larger by N every iteration — and it used
 * to be reallocated to the exact size EVERY iteration: a hipFree (which waits for every stream of the device: the generator's, when it
 * works ahead on a stream of its own — why round 4's sample prefetch never overlapped anything, profiles/r04_mlsl_prefetch_timeline.txt) and
 * a hipMalloc of tens of MB between the sampling kernel and the distance pass.  Now it doubles: a handful of reallocations per run.
 * One rule for both scratch matrices (d_D, and d_D2 of the sampling phase enqueued ahead). */
static int grow_scratch(mlsl_dev *d, double **buf, size_t *cap, size_t doubles, const char *what)
{
    if (doubles <= *cap) return 0;
    if (doubles < 2 * *cap) doubles = 2 * *cap;
    if (!*cap) {               /* the first allocation: the pass of the 8th iteration (N x 8 N doubles, within 1 GiB) */
        const size_t want = 8 * (size_t) d->N * (size_t) d->N, budget = ((size_t) 1 << 30) / sizeof(double);
        if (doubles < (want < budget ? want : budget)) doubles = want < budget ? want : budget;
    }
    nla_dev_free(*buf);
    *buf = (double *) nla_dev_malloc(sizeof(double) * doubles);
    *cap = *buf ? doubles : 0;
    if (!*buf) MFAIL(d, "out of device memory (%s)", what);
    return 0;
}
static int need_D(mlsl_dev *d, size_t doubles) { return grow_scratch(d, &d->d_D, &d->dcap, doubles, "distance matrix"); }

/* ---- the device passes of a sampling phase: one copy each, for the iteration's own phase (stream st, scratch d_D) and for the one
 * enqueued ahead (stream rs, scratch d_D2).  r0, mine: the block of the N new rows this rank computes — all of them on one rank ---- */

/* f of `cnt` rows on the device: compiled-in objective, or the user's kernel (host objectives are called by the host walks) */
static int mlsl_eval_rows(mlsl_dev *d, const double *rows, int cnt, double *dF, void *stream)
{
    if (d->ev.kind == NLA_EVAL_USER) return nla_userobj_eval_rows(d->ev.user, d->n, d->ld, cnt, rows, dF, NULL, d->ev.sign, stream);
    return nla_k_eval(d->obj, d->n, d->ld, rows, cnt, dF, stream) || (d->ev.sign < 0 && nla_k_mlsl_negate(dF, cnt, stream));
}

/* the N sample rows first .. first + N - 1 and, with `evaluate`, their f (mlsl.c:355-360): Sobol points by index, or the stream's words
 * (nlopt_urand) — that kernel evaluates a compiled-in objective itself, and a device objective is evaluated on this path whether or
 * not the host walk replaces the values afterwards (the host search on a device objective), as it always was */
static int mlsl_sample_rows(mlsl_dev *d, void *stream, size_t first, int evaluate)
{
    double *rows = d->d_P + first * (size_t) d->ld, *F = d->d_F + first;
    if (d->d_V)                                                                /* nlopt_sobol_next, mlsl.c:355 */
        return nla_k_mlsl_sobol_rows(d->n, d->ld, d->d_lb, d->d_ub, d->d_V, d->sobol_next, d->N, rows, stream) ||
               (evaluate && mlsl_eval_rows(d, rows, d->N, F, stream));
    if (nla_k_crs_init_rows(d->obj, d->n, d->ld, d->d_lb, d->d_ub, d->d_words, (int64_t) first, d->N, d->d_P, d->d_F, stream)) return -1;
    if (d->ev.kind == NLA_EVAL_DEVICE) return d->ev.sign < 0 && nla_k_mlsl_negate(F, d->N, stream);
    return d->ev.kind == NLA_EVAL_USER && mlsl_eval_rows(d, rows, d->N, F, stream);
}

/* closest_pt_d of the new points old .. old + N - 1: over every point with smaller f; of the old, not yet minimised points: over the new
 * points with smaller f (find_closest_pt, pts_update_newpt: mlsl.c:155-178).  Several ranks: the ROWS of the new points are dealt in
 * blocks over the ranks; every rank computes its rows' minima and its rows' share of the column minima, combined by an element-wise
 * min over an all-gather (exact).  cpd: the nb = old + N minima on the device; minimized: the flags, or NULL = none is */
static int mlsl_closest_pt_pass(mlsl_dev *d, void *stream, size_t old, int r0, int mine, double *D, double *cpd, const int32_t *minimized)
{
    const int nb = (int) (old + (size_t) d->N);
    const double *A = d->d_P + (old + (size_t) r0) * (size_t) d->ld, *FA = d->d_F + old + r0;
    return mine > 0 && (nla_k_mlsl_dist2(d->n, d->ld, A, mine, d->d_P, nb, D, stream) ||
                        nla_k_mlsl_rowmin(D, nb, mine, nb, FA, d->d_F, NULL, cpd + old + r0, stream) ||
                        nla_k_mlsl_colmin(D, nb, mine, (int) old, FA, d->d_F, minimized, cpd, stream));
}

/* closest_lm_d of the same rows over the minima l0 .. l0 + lc - 1 (find_closest_lm, mlsl.c:139-153), into h_out[0 .. mine) */
static int mlsl_closest_lm_pass(mlsl_dev *d, void *stream, size_t old, int r0, int mine, size_t l0, size_t lc, double *D, double *d_out, double *h_out)
{
    const double *A = d->d_P + (old + (size_t) r0) * (size_t) d->ld, *FA = d->d_F + old + r0;
    return mine > 0 && lc && (nla_k_mlsl_dist2(d->n, d->ld, A, mine, d->d_LM + l0 * (size_t) d->ld, (int) lc, D, stream) ||
                              nla_k_mlsl_rowmin(D, (int) lc, mine, (int) lc, FA, d->d_LF + l0, NULL, d_out, stream) ||
                              nla_memcpy_d2h(h_out, d_out, sizeof(double) * (size_t) mine, stream));
}

/* ---- the next iteration's sampling phase, ahead (see mlsl_dev) ---- */
static int ahead_buffers(mlsl_dev *d, size_t doubles)
{
    if (d->cap2 < d->cap) {
        size_t i;
        nla_host_free(d->h_cpd2); nla_host_free(d->h_inf); nla_dev_free(d->d_cpd2);
        d->h_cpd2 = (double *) nla_host_malloc(sizeof(double) * d->cap);
        d->h_inf = (double *) nla_host_malloc(sizeof(double) * d->cap);
        d->d_cpd2 = (double *) nla_dev_malloc(sizeof(double) * d->cap);
        d->cap2 = (d->h_cpd2 && d->h_inf && d->d_cpd2) ? d->cap : 0;
        if (!d->cap2) MFAIL(d, "out of memory (sampling ahead)");
        for (i = 0; i < d->cap; ++i) d->h_inf[i] = HUGE_VAL;
    }
    if (!d->Fnew2) d->Fnew2 = (double *) nla_host_malloc(sizeof(double) * (size_t) d->N);
    if (!d->h_cld2) d->h_cld2 = (double *) nla_host_malloc(sizeof(double) * (size_t) d->N);
    if (!d->d_cld2) d->d_cld2 = (double *) nla_dev_malloc(sizeof(double) * (size_t) d->N);
    if (!d->Fnew2 || !d->h_cld2 || !d->d_cld2) MFAIL(d, "out of memory (sampling ahead)");
    return grow_scratch(d, &d->d_D2, &d->dcap2, doubles, "distance matrix of the samples ahead");
}

/* enqueue, on the generator's stream, the sampling of the iteration AFTER the current one: rows npts .. npts + N - 1 (the current
 * iteration's sampling is complete, its local phase adds no points), their values, closest_pt_d of and through them (find_closest_pt,
 * pts_update_newpt: mlsl.c:155-178) and their closest_lm_d over the minima known now (find_closest_lm, :139-153).  Called in front of
 * the local searches' launch, behind the generator's fill of the words these rows are made of.  Every allocation it may need is
 * made here, before anything is enqueued (freeing device memory waits for the whole device). */
static int mlsl_enqueue_ahead(mlsl_dev *d)
{
    const size_t old = d->npts, nlms = d->nlms;
    const int N = d->N, nb = (int) (old + (size_t) N);
    const size_t cols = (size_t) nb > nlms ? (size_t) nb : nlms;
    d->ahead_valid = 0;
    if (d->d_V && (uint64_t) d->sobol_next + (uint64_t) N >= 4294967295ULL) return 0;     /* (the iteration itself reports the exhausted sequence) */
    if ((size_t) N * cols > ((size_t) 1 << 29)) { d->ahead = 0; return 0; }               /* a second distance matrix above 4 GiB: not worth the memory */
    if (grow_pts(d, old + (size_t) N) || ahead_buffers(d, (size_t) N * cols)) return -1;
    if (d->h_gate_gave_up && *(volatile int32_t *) d->h_gate_gave_up) {     /* (the launch it belonged to has long ended) */
        *(volatile int32_t *) d->h_gate_gave_up = 0; d->gate_off = 1;
        if (d->stats) ++d->stats->mlsl_gate_timeouts;
    }
    if (d->gate_need > 0 && !d->gate_off && nla_k_gate(d->gate_counter, d->gate_from, d->gate_need, 50.0, d->h_gate_gave_up, d->rs)) MFAIL(d, "sampling ahead failed");
    if (mlsl_sample_rows(d, d->rs, old, 1)) MFAIL(d, "sampling ahead failed");
    if (nla_memcpy_d2h(d->Fnew2, d->d_F + old, sizeof(double) * (size_t) N, d->rs) ||
        nla_memcpy_h2d(d->d_cpd2, d->h_inf, sizeof(double) * (size_t) nb, d->rs) ||
        mlsl_closest_pt_pass(d, d->rs, old, 0, N, d->d_D2, d->d_cpd2, NULL) ||
        nla_memcpy_d2h(d->h_cpd2, d->d_cpd2, sizeof(double) * (size_t) nb, d->rs) ||
        mlsl_closest_lm_pass(d, d->rs, old, 0, N, 0, nlms, d->d_D2, d->d_cld2, d->h_cld2) ||
        nla_event_record(d->ev_ahead, d->rs)) MFAIL(d, "distance pass ahead failed");
    d->ahead_old = old; d->ahead_nlms = nlms; d->ahead_words = d->words_used; d->ahead_sobol = d->sobol_next;
    d->ahead_valid = 1;
    return 0;
}

/* insert row id `r` (value f) into an order array: before the first element that is not smaller */
static void ord_insert(size_t *ord, size_t cnt, const double *F, size_t r)
{
    size_t lo = 0, hi = cnt;
    const double f = F[r];
    while (lo < hi) { size_t mid = (lo + hi) / 2; if (F[ord[mid]] < f) lo = mid + 1; else hi = mid; }
    memmove(ord + lo + 1, ord + lo, (cnt - lo) * sizeof *ord);
    ord[lo] = r;
}

/* the same for a run of nnew consecutive rows first .. first + nnew - 1 inserted one after the other (the sampling phase's 1000 points
 * per iteration: a binary search through F and a memmove of half the array each — 1 ms per iteration at 3000 points, growing with the
 * point set): sort the new rows, merge from the back.  The order is the one-by-one insertion's: an equal key goes in front of those
 * already there, so among equals new rows come before old ones and later new rows before earlier ones.  (Keys that do not order —
 * NaN — take the one-by-one path: the binary search's answer for them is whatever it happens to be, and that is what counts.) */
static int ord_cmp_new(const void *a_, const void *b_, void *F_)
{
    const double *F = (const double *) F_;
    const size_t a = *(const size_t *) a_, b = *(const size_t *) b_;
    if (F[a] < F[b]) return -1;
    if (F[a] > F[b]) return 1;
    return a > b ? -1 : (a < b ? 1 : 0);                 /* the later row first */
}
static void ord_insert_run(size_t *ord, size_t cnt, const double *F, size_t first, size_t nnew, int any_nan)
{
    size_t k;
    long i, j;
    for (k = 0; k < nnew && !any_nan; ++k) if (F[first + k] != F[first + k]) any_nan = 1;
    if (any_nan || nnew < 8) { for (k = 0; k < nnew; ++k) ord_insert(ord, cnt + k, F, first + k); return; }
    for (k = 0; k < nnew; ++k) ord[cnt + k] = first + k;                      /* the tail of the array is the merge's scratch */
    qsort_r(ord + cnt, nnew, sizeof *ord, ord_cmp_new, (void *) F);
    {
        /* merge in place from the back; the sorted new rows are first moved out of the way of the write position */
        size_t *tmp = (size_t *) malloc(sizeof *tmp * nnew);
        if (!tmp) { for (k = 0; k < nnew; ++k) ord[cnt + k] = 0; for (k = 0; k < nnew; ++k) ord_insert(ord, cnt + k, F, first + k); return; }
        memcpy(tmp, ord + cnt, sizeof *tmp * nnew);
        i = (long) cnt - 1; j = (long) nnew - 1;
        for (k = cnt + nnew; k-- > 0 && j >= 0; ) {
            if (i >= 0 && !(F[ord[i]] < F[tmp[j]])) ord[k] = ord[i--];       /* an old row with a key not smaller stays behind the new one */
            else ord[k] = tmp[j--];
        }
        free(tmp);
    }
}

/* the distances of a batch's minimisers to every point + the nb x nb of them the commit walk reads, enqueued on the stream (MLSL's
 * local phase; with a device objective on one rank: right behind the searches' kernel, nla_local_ctx_after_launch) */
typedef struct { mlsl_dev *d; int nb; size_t na; const double *ctx_X; size_t lx_bytes; } mlsl_pairs_job;
static int mlsl_enqueue_pairs(void *arg)
{
    mlsl_pairs_job *j = (mlsl_pairs_job *) arg;
    mlsl_dev *d = j->d;
    if (j->ctx_X && j->lx_bytes && nla_memcpy_d2d(d->d_LX, j->ctx_X, j->lx_bytes, d->st)) return -1;      /* (one rank: the all-gather of the minimisers is this copy) */
    return nla_memcpy_h2d(d->d_gi, d->h_gi, sizeof(int64_t) * (size_t) j->nb, d->st) ||
           nla_k_mlsl_dist2(d->n, d->ld, d->d_LX, (int) j->na, d->d_P, (int) d->npts, d->d_D, d->st) ||
           nla_k_mlsl_gather_pairs_t(d->d_D, (int) d->npts, d->d_gi, j->nb, d->d_idx, j->nb, d->d_S, d->st) ||
           nla_memcpy_d2h(d->h_S, d->d_S, sizeof(double) * (size_t) j->nb * (size_t) j->nb, d->st);
}

/* v[k] = min over the ranks of their v[k] (each rank holds the minima over ITS rows of the distance matrix) */
static int min_over_ranks(mlsl_dev *d, double *v, size_t count)
{
    size_t k;
    int r;
    if (count == 0) return 0;
    if ((size_t) d->world * count > d->gcap) {
        free(d->h_gather);
        d->gcap = 2 * (size_t) d->world * count;
        d->h_gather = (double *) malloc(sizeof(double) * d->gcap);
        if (!d->h_gather) { d->gcap = 0; return -1; }
    }
    if (nla_comm_allgather_host(d->comm, v, d->h_gather, sizeof(double) * count, d->st)) return -1;
    for (k = 0; k < count; ++k) {
        double m = d->h_gather[k];
        for (r = 1; r < d->world; ++r) { const double t = d->h_gather[(size_t) r * count + k]; if (t < m) m = t; }
        v[k] = m;
    }
    return 0;
}

/* the objective as MLSL's local optimiser sees it (mlsl_count_wrap) */
static double mlsl_counted_f(unsigned n, const double *x, double *grad, void *p)
{
    mlsl_count_wrap *w = (mlsl_count_wrap *) p;
    ++*w->nevals_p;
    return w->f(n, x, grad, w->f_data);
}
/* -f for a maximisation whose objective the dispatcher left unflipped (dev_sign) but which runs through host calls here */
static double mlsl_signed_f(unsigned n, const double *x, double *grad, void *p)
{
    mlsl_count_wrap *w = (mlsl_count_wrap *) p;
    (void) grad;
    return w->sign * w->f(n, x, NULL, w->f_data);
}


/* ---- small pieces every phase uses ---- */
static const double dlm = 1.0, dbound = 1e-6;             /* mlsl.c:324-325 */

/* candidate c of a batch is minimised by rank c mod world in its slot c / world (`per` slots per rank): its gathered row */
static inline size_t mlsl_gi(int c, int world, int per) { return (size_t) (c % world) * (size_t) per + (size_t) (c / world); }

static int mlsl_agree(mlsl_dev *d)
{
    d->sp = nla_comm_agree_stop(d->comm, d->stop, &d->agreed_view, &d->agreed_force);
    if (!d->sp) MFAIL(d, "stop agreement failed: %s", nlopt_amd_comm_error(d->comm));
    return 0;
}

/* The three stop-test sequences differ in order ON PURPOSE: each restates the reference's lines named with it.
 * After a sample (mlsl.c:340-343 for the first point, :365-368): forced, evals, time, minf */
static nlopt_result mlsl_stop_after_sample(const mlsl_dev *d, double fv)
{
    if (nla_stop_forced(d->sp)) return NLOPT_FORCED_STOP;
    if (nla_stop_evals(d->stop)) return NLOPT_MAXEVAL_REACHED;
    if (nla_stop_time(d->sp)) return NLOPT_MAXTIME_REACHED;
    if (fv < d->stop->minf_max) return NLOPT_MINF_MAX_REACHED;
    return NLOPT_SUCCESS;
}
/* after a local search, when its minimum is committed (mlsl.c:413-419): forced, minf, evals, time */
static nlopt_result mlsl_stop_after_search(const mlsl_dev *d, double lf)
{
    if (nla_stop_forced(d->sp)) return NLOPT_FORCED_STOP;
    if (lf < d->stop->minf_max) return NLOPT_MINF_MAX_REACHED;
    if (nla_stop_evals(d->stop)) return NLOPT_MAXEVAL_REACHED;
    if (nla_stop_time(d->sp)) return NLOPT_MAXTIME_REACHED;
    return NLOPT_SUCCESS;
}
/* in front of a search whose callbacks the caller sees (mlsl.c:391-399; one process): forced, evals, and the raw clock of the
 * caller's own `stop`, not of the agreed view */
static nlopt_result mlsl_stop_before_host_search(const mlsl_dev *d)
{
    const nla_stopping *stop = d->stop;
    if (nla_stop_forced(stop)) return NLOPT_FORCED_STOP;
    if (nla_stop_evals(stop)) return NLOPT_MAXEVAL_REACHED;
    if (stop->maxtime > 0 && nla_seconds() - stop->start >= stop->maxtime) return NLOPT_MAXTIME_REACHED;
    return NLOPT_SUCCESS;
}

/* the evaluation limit of the next local search (nlopt_optimize_limited, optimize.c:1097-1100) */
static int mlsl_eval_limit(const mlsl_dev *d)
{
    const long limited = (long) d->stop->maxeval - (long) *d->stop->nevals_p;
    int eff = d->loc_maxeval;
    if (d->loc_maxeval <= 0 || (limited > 0 && limited < d->loc_maxeval)) eff = (int) limited;
    return eff;
}

static void mlsl_trace(nlopt_opt opt, double f, size_t row, int kind, int accepted)
{
    if (!opt || !opt->trace) return;
    if (opt->trace_len < opt->trace_cap) { nlopt_amd_trace_rec *tr = opt->trace + opt->trace_len; tr->f = f; tr->row = (int64_t) row; tr->kind = kind; tr->accepted = accepted; }
    ++opt->trace_len;
}

static void mlsl_get_minf(mlsl_dev *d)                                         /* get_minf, mlsl.c:258-274 */
{
    if (d->npts) { d->best_f = d->F[d->ord[0]]; d->best_row = d->ord[0]; d->best_is_lm = 0; }
    if (d->nlms && d->LF[d->lord[0]] < d->best_f) { d->best_f = d->LF[d->lord[0]]; d->best_row = d->lord[0]; d->best_is_lm = 1; }
}

/* what waits for the next launch of local searches (see the end of mlsl_sampling_phase): the generator's fill of the next iteration's
 * words, and that iteration's sampling phase behind it */
static int mlsl_prefetch_now(mlsl_dev *d)
{
    if (d->prefetch_due) {
        d->prefetch_due = 0;
        if (nla_mtstream_fill(d->mts, d->words_used, 2ULL * (uint64_t) d->n * (uint64_t) d->N, d->d_words)) MFAIL(d, "MT stream fill failed");
        d->prefetched_at = d->words_used;
    }
    if (d->ahead_due) { d->ahead_due = 0; if (mlsl_enqueue_ahead(d)) return -1; }
    return 0;
}

/* ---- set-up ---- */

/* the arguments the reference checks (mlsl.c:283-297), and the local optimisers this library provides */
static nlopt_result mlsl_check_args(mlsl_dev *d, nla_stopping *stop, nlopt_opt local_opt, int Nsamples)
{
    int rc;
    d->N = Nsamples ? Nsamples : 4;                                            /* mlsl.c:283-286 */
    if (d->N < 1) { nla_stop_msg(stop, "population %d is too small", d->N); return NLOPT_INVALID_ARGS; }
    if (!local_opt || (local_opt->algorithm != NLOPT_LD_LBFGS && local_opt->algorithm != NLOPT_LD_MMA && local_opt->algorithm != NLOPT_LN_COBYLA)) {
        nla_stop_msg(stop, "nlopt_amd: MLSL is provided with NLOPT_LD_LBFGS, NLOPT_LD_MMA or NLOPT_LN_COBYLA as the local optimizer only (not %s)",
                     local_opt ? nlopt_algorithm_name(local_opt->algorithm) : "none");
        return NLOPT_INVALID_ARGS;
    }
    if (local_opt->algorithm == NLOPT_LD_MMA && (rc = nla_mma_read_params(local_opt, &d->mma))) {
        nla_stop_msg(stop, "%s", local_opt->errmsg ? local_opt->errmsg : "invalid LD_MMA parameter");
        return (nlopt_result) rc;
    }
    return NLOPT_SUCCESS;
}

/* Who runs the local searches (d->ev is resolved).  LD_LBFGS and LD_MMA: their batched kernels.
 * LN_COBYLA (GN_MLSL's default, optimize.c:763-768).  With a compiled-in device objective (round 6) the searches of a batch run
 * CONCURRENTLY on the device, one wavefront per start, like LD_LBFGS / LD_MMA: MLSL_DEV_COBYLA.  The search's whole state is in LDS while
 * it fits a compute unit's (n <= 51, hip/cobyla_kernels.hip); beyond, up to NLA_COBYLA_GLOBAL_MAX_N, its matrices are in device
 * memory (hip/cobyla_global.hip) — the same search, local_ctx.c picks the launcher.  With a user-supplied device objective
 * (NLA_EVAL_USER) on one process, n <= NLA_COBYLA_GLOBAL_MAX_N, the same again as a coroutine (hip/cobyla_ext.hip): the waiting
 * searches of a batch are evaluated by ONE launch of the user's kernel per step (nla_local_ctx_run), and everything else
 * is the compiled-in case's.  Otherwise — a host callback, a user kernel on several ranks (nothing there to check it
 * against), a dimension beyond the kernels (or a device layer without them), or "amd_cobyla_host" = 1 on either object — it is a HOST
 * algorithm (cobyla_host.c), MLSL_HOST_SEARCH: the searches run one at a time on the caller's thread through the library's own
 * nlopt_optimize, exactly as mlsl.c:404-407 runs them; samples, distances and the bookkeeping stay on the device, and the run takes the
 * host-callback path throughout. */
static mlsl_local mlsl_choose_local(const mlsl_dev *d, nlopt_opt opt, nlopt_opt local_opt, const double *lb, const double *ub)
{
    int i, dev;
    if (local_opt->algorithm == NLOPT_LD_MMA) return MLSL_MMA;
    if (local_opt->algorithm != NLOPT_LN_COBYLA) return MLSL_LBFGS;
    dev = nla_cobyla_device_serves(d->ev.kind, d->n) && (d->ev.kind == NLA_EVAL_DEVICE || nlopt_amd_comm_world(opt ? opt->comm : NULL) == 1) &&
          !(opt && nlopt_get_param(opt, "amd_cobyla_host", 0) != 0) && !nlopt_get_param(local_opt, "amd_cobyla_host", 0);
    /* a fixed coordinate (lb[i] == ub[i]): the reference's nlopt_optimize_limited eliminates it in front of each COBYLA search
     * (optimize.c:412-445), the device kernel does not (it refuses such a box, include/nlopt_amd.h) — the host algorithm, whose
     * nlopt_optimize eliminates like the reference (api_optimize.c fix_applies) */
    for (i = 0; dev && i < d->n; ++i) if (lb[i] == ub[i]) dev = 0;
    return dev ? MLSL_DEV_COBYLA : MLSL_HOST_SEARCH;
}

/* Everything a run needs before its first evaluation.  ONE failure exit: the message, "not ready" to the other ranks (several ranks:
 * set-up ends with an exchange of "ready" — comm.c, nla_comm_agree_ready — and a rank that fails here says so there instead of
 * leaving the others in the run's first collective), the result code.  The caller tears down (mfree) whatever was made. */
static nlopt_result mlsl_setup(mlsl_dev *d, nlopt_opt opt, int n, nlopt_func f, void *f_data, const double *lb, const double *ub,
                               nla_stopping *stop, nlopt_opt local_opt, int lds)
{
    const char *msg = "nlopt_amd: could not create the MLSL device state";
    nlopt_result code = NLOPT_OUT_OF_MEMORY;
    nlopt_amd_stats *st = opt ? &opt->stats : NULL;
    int i, bmax;

    d->opt = opt; d->local_opt = local_opt; d->stop = stop; d->sp = stop; d->stats = st;
    d->n = n; d->ld = (n + 1) & ~1;
    if (nla_dev_count() <= 0) {
        /* (asked before the searches are placed: with LN_COBYLA, host or device, this exit has never told the other ranks) */
        d->comm = (opt && local_opt->algorithm != NLOPT_LN_COBYLA) ? opt->comm : NULL;
        msg = "nlopt_amd: no HIP device visible (this library has no CPU fallback)"; code = NLOPT_FAILURE;
        goto fail;
    }
    nla_evaluator_resolve(&d->ev, opt, f, f_data);
    d->obj = d->ev.kind == NLA_EVAL_DEVICE ? d->ev.obj : -1;
    d->local = mlsl_choose_local(d, opt, local_opt, lb, ub);
    d->host = d->ev.kind == NLA_EVAL_HOST || d->local == MLSL_HOST_SEARCH;
    d->sw.f = f; d->sw.f_data = f_data; d->sw.sign = -1.; d->sw.nevals_p = NULL;
    if (d->local == MLSL_HOST_SEARCH && d->ev.kind != NLA_EVAL_HOST && d->ev.sign < 0) { f = mlsl_signed_f; f_data = &d->sw; }   /* a maximisation the dispatcher left unflipped (dev_sign): flip here */
    d->f = f; d->f_data = f_data;
    d->comm = (opt && d->local != MLSL_HOST_SEARCH) ? opt->comm : NULL;       /* host searches: every rank runs the identical job, nothing to exchange */
    d->world = nlopt_amd_comm_world(d->comm); d->rank = nlopt_amd_comm_rank(d->comm);
    d->batch = d->host ? 1 : BATCH_MAX;       /* a host callback is called for one search at a time, in the reference's order */
    d->bmax = bmax = d->batch * d->world;
    /* what a local search observes of the caller's stopping state: the force_stop flag and the run's clock
     * (nlopt_optimize_limited hands the remaining time down, optimize.c:1101-1104) */
    d->lstop = *stop;
    d->lstop.xtol_abs = local_opt->xtol_abs; d->lstop.x_weights = local_opt->x_weights;
    d->R_prefactor = sqrt(2. / K2PI) * pow(gam(n) * MLSL_SIGMA, 1.0 / n);        /* mlsl.c:313-317 */
    for (i = 0; i < n; ++i) d->R_prefactor *= pow(ub[i] - lb[i], 1.0 / n);
    d->best_f = HUGE_VAL;

    /* the local optimiser as nlopt_optimize_limited(local_opt, ...) would configure it (mlsl.c:303-306,404-407) */
    d->prm.minf_max = stop->minf_max; d->prm.ftol_rel = local_opt->ftol_rel; d->prm.ftol_abs = local_opt->ftol_abs;
    d->prm.xtol_rel = local_opt->xtol_rel; d->prm.tolg = nlopt_get_param(local_opt, "tolg", 0.);
    d->loc_maxeval = local_opt->maxeval;

    d->st = nla_stream_create();
    /* PREFETCH (always, with a device objective; measured on the MI355X in round 5 together with the short segments below: config 4
     * 15.9 -> 13.9 ms per iteration, profiles/r05_staged_ab.txt): pseudo-random sampling (every MLSL
     * variant at n > 1111, where the reference has no Sobol generator either) costs a generator pass per iteration that is bound by
     * latency, not throughput — 2 n N words are 13 segments = 13 wavefronts at config 4, 1.9 ms + 0.5-1 ms of segment jumps of the
     * 7.5 ms sampling phase.  Nothing between two sampling phases draws random numbers (the local optimisers are deterministic), so
     * the NEXT iteration's words are generated on a stream of their own beside the distance pass and the local searches.  Hand-over
     * = a host synchronisation of that stream before the sampling kernel reads them. */
    d->prefetch = !d->host;
    /* (not with the sums in the reference's order, amd_exact_dot = 1: that launch is one chain of dependent fp64 additions per search,
     * every issue slot the distance pass takes on its SIMD delays the chain — measured: 103 -> 117 ms per launch, round 5) */
    d->ahead = !d->host && d->world == 1 && d->ev.kind == NLA_EVAL_DEVICE && d->local != MLSL_DEV_COBYLA && !nla_exact_mode_for(opt, local_opt, &d->ev);
    d->prefetched_at = ~0ULL;
    if (d->ahead) { d->h_gate_gave_up = (int32_t *) nla_host_malloc(sizeof(int32_t)); if (d->h_gate_gave_up) *d->h_gate_gave_up = 0; }     /* (its failure is found below) */
    d->rs = (d->st && d->prefetch) ? nla_stream_create_background() : d->st;
    d->ev_samples = nla_event_create();
    d->ev_ahead = nla_event_create();
    {
        /* "amd_mlsl_seg_regens": the segment length of this run's stream (NLA_MT_SEG_REGENS = 1024 is the layout every other algorithm
         * uses) — 64 makes 205 wavefronts of the 13 above; measured at config 4 (MI355X, round 5): 15.9 ms per iteration at 1024, 14.7 at
         * 256, 14.4 at 64, 14.3 at 16.  The words are the same. */
        int seg = opt ? (int) nlopt_get_param(opt, "amd_mlsl_seg_regens", NLA_MLSL_SEG_REGENS) : NLA_MLSL_SEG_REGENS;
        if (seg < 1 || seg > NLA_MT_SEG_REGENS || (seg & (seg - 1))) seg = NLA_MT_SEG_REGENS;
        if (d->st && d->rs) d->mts = seg == NLA_MT_SEG_REGENS ? nla_mtstream_create(d->rs) : nla_mtstream_create_seg(d->rs, seg);
    }
    if (!d->st || !d->rs || !d->mts) { msg = "nlopt_amd: could not create the device stream / generator state"; goto fail; }
    d->d_lb = (double *) nla_dev_malloc(sizeof(double) * (size_t) d->ld);
    d->d_ub = (double *) nla_dev_malloc(sizeof(double) * (size_t) d->ld);
    d->d_words = (uint32_t *) nla_dev_malloc(sizeof(uint32_t) * 2 * (size_t) n * (size_t) d->N);
    d->d_tmp = (double *) nla_dev_malloc(sizeof(double) * (size_t) (d->N > bmax ? d->N : bmax));
    d->d_LX = (double *) nla_dev_malloc(sizeof(double) * (size_t) bmax * (size_t) d->ld);
    d->h_idx = (int64_t *) nla_host_malloc(sizeof(int64_t) * (size_t) (2 * bmax + BATCH_MAX));
    d->d_idx = (int64_t *) nla_dev_malloc(sizeof(int64_t) * (size_t) (2 * bmax + BATCH_MAX));
    d->h_lf = (double *) nla_host_malloc(sizeof(double) * (size_t) bmax);
    d->h_S = (double *) nla_host_malloc(sizeof(double) * (size_t) bmax * (size_t) bmax);
    d->d_S = (double *) nla_dev_malloc(sizeof(double) * (size_t) bmax * (size_t) bmax);
    d->h_lfall = (double *) nla_host_malloc(sizeof(double) * (size_t) bmax);
    d->lf_cand = (double *) malloc(sizeof(double) * (size_t) bmax);
    d->d_lfall = (double *) nla_dev_malloc(sizeof(double) * (size_t) bmax);
    d->h_gi = (int64_t *) nla_host_malloc(sizeof(int64_t) * (size_t) bmax);
    d->d_gi = (int64_t *) nla_dev_malloc(sizeof(int64_t) * (size_t) bmax);
    d->h_flags = (int32_t *) nla_host_malloc(sizeof(int32_t) * (size_t) bmax);
    d->d_flags = (int32_t *) nla_dev_malloc(sizeof(int32_t) * (size_t) bmax);
    d->Fnew = (double *) nla_host_malloc(sizeof(double) * (size_t) d->N);
    if (d->host) d->h_rows = (double *) nla_host_malloc(sizeof(double) * (size_t) d->N * (size_t) d->ld);
    d->res = (nla_lbfgs_result *) malloc(sizeof *d->res * (size_t) bmax);
    d->res_mine = (nla_lbfgs_result *) calloc(BATCH_MAX, sizeof *d->res_mine);
    d->cand = (size_t *) malloc(sizeof *d->cand * (size_t) bmax);
    if ((d->host && !d->h_rows) || !d->h_idx || !d->d_idx || !d->h_lf || !d->h_S || !d->d_S || !d->h_lfall || !d->lf_cand || !d->d_lfall || !d->h_gi || !d->d_gi ||
        !d->h_flags || !d->d_flags || !d->d_lb || !d->d_ub || !d->d_words || !d->d_tmp || !d->d_LX || !d->ev_samples || !d->ev_ahead || (d->ahead && !d->h_gate_gave_up) ||
        !d->Fnew || !d->res || !d->res_mine || !d->cand || grow_pts(d, (size_t) d->N + 1) || grow_lms(d, 1) ||
        nla_memcpy_h2d(d->d_lb, lb, sizeof(double) * (size_t) n, d->st) || nla_memcpy_h2d(d->d_ub, ub, sizeof(double) * (size_t) n, d->st)) goto fail;
    if (lds) {                                                                 /* d.s = nlopt_sobol_create(n), mlsl.c:306 */
        uint32_t *V = (uint32_t *) malloc(sizeof(uint32_t) * 32 * (size_t) n);
        int bad = 0;
        if (V && nla_sobol_directions((unsigned) n, V)) {
            d->d_V = (uint32_t *) nla_dev_malloc(sizeof(uint32_t) * 32 * (size_t) n);
            bad = !d->d_V || nla_memcpy_h2d(d->d_V, V, sizeof(uint32_t) * 32 * (size_t) n, d->st) || nla_stream_sync(d->st);
            d->sobol_next = nla_sobol_skip_count((unsigned) (10 * n + d->N)) + 1;  /* nlopt_sobol_skip(d.s, 10n+N, .), mlsl.c:332 */
        }                                                                      /* else: NULL generator -> nlopt_urand, as the reference */
        free(V);
        if (bad) goto fail;
    }
    if ((d->local == MLSL_MMA || d->local == MLSL_DEV_COBYLA) && local_opt->dx) {                /* the initial step = MMA's sigma_init, optimize.c:829 */
        d->d_dx = (double *) nla_dev_malloc(sizeof(double) * (size_t) d->ld);
        if (!d->d_dx || nla_memcpy_h2d(d->d_dx, local_opt->dx, sizeof(double) * (size_t) n, d->st) || nla_stream_sync(d->st)) goto fail;
    }
    if (d->local == MLSL_HOST_SEARCH) {
        /* the local optimiser as mlsl.c:303-306 configures it: counted objective, the box, the stop value */
        d->lo_f = local_opt->f; d->lo_fdata = local_opt->f_data;
        d->cw.f = f; d->cw.f_data = f_data; d->cw.sign = 1.; d->cw.nevals_p = stop->nevals_p;      /* (f is already the flipped one where that applies) */
        /* installed by assignment and taken out again by mfree, on every exit (opt->local_opt is the object's own copy whose objective
         * nlopt_set_local_optimizer cleared, options.c:824-846: nothing of the user's to munge, but nothing of the caller's stack frame
         * may stay behind in it either) */
        local_opt->f = mlsl_counted_f; local_opt->f_data = &d->cw; local_opt->pre = NULL; local_opt->maximize = 0;
        d->lo_installed = 1;
        nlopt_set_lower_bounds(local_opt, lb);
        nlopt_set_upper_bounds(local_opt, ub);
        nlopt_set_stopval(local_opt, stop->minf_max);
        d->cob_x = (double *) nla_host_malloc(sizeof(double) * (size_t) n);
        if (!d->cob_x) { msg = "nlopt_amd: out of pinned memory"; goto fail; }
    } else {
        const int use_mma = d->local == MLSL_MMA;
        const nla_local_spec spec = { d->local == MLSL_DEV_COBYLA ? NLA_LOCAL_COBYLA : use_mma ? NLA_LOCAL_MMA : NLA_LOCAL_LBFGS, &d->ev, n, d->batch,
                                      nla_lbfgs_default_mf(n, (int) local_opt->vector_storage, 0), use_mma ? &d->mma : NULL, d->d_dx, d->d_lb, d->d_ub, d->st,
                                      NULL, 0, 0, 0, 0, NULL, NULL };      /* (MLSL strips its local optimiser's nonlinear constraints, options.c:824-846) */
        d->lb = nla_local_ctx_create(&spec);
        if (d->lb && nla_local_ctx_set_options(d->lb, nla_exact_mode_for(opt, local_opt, &d->ev), local_opt->xtol_abs, local_opt->x_weights)) { nla_local_ctx_destroy(d->lb); d->lb = NULL; }
        /* (LD_LBFGS only: LD_MMA's launches are half as long as the distance pass beside them — behind a gate it ends after them and holds the
         * next iteration up: config 4 with LD_MMA 8.0 -> 8.3 ms per iteration, profiles/r05_mlsl_ahead_ab.txt) */
        if (d->lb && d->ahead && !use_mma && NLA_MLSL_GATE_PCT > 0 && nla_local_ctx_count_finished(d->lb)) { nla_local_ctx_destroy(d->lb); d->lb = NULL; }
        if (!d->lb) { msg = "nlopt_amd: out of device memory (local-search batch)"; goto fail; }
        nla_local_ctx_set_stats(d->lb, st);
        if (d->local == MLSL_DEV_COBYLA) nla_local_ctx_set_cobyla_min_batch(d->lb, (int) nlopt_get_param(opt ? opt : local_opt, "amd_cobyla_min_batch", nlopt_get_param(local_opt, "amd_cobyla_min_batch", 0)));
    }
    return NLOPT_SUCCESS;
fail:
    nla_stop_msg(stop, "%s", msg);
    nla_comm_agree_ready(d->comm, 0);
    return code;
}

/* ---- the starting guess is the first point (mlsl.c:326-343) ---- */
static int mlsl_first_point(mlsl_dev *d, const double *x)
{
    const size_t xbytes = sizeof(double) * (size_t) d->n;
    if (d->host) {
        d->F[0] = d->f((unsigned) d->n, x, NULL, d->f_data);
        if (nla_memcpy_h2d(d->d_P, x, xbytes, d->st) || nla_memcpy_h2d(d->d_F, d->F, sizeof(double), d->st) ||
            nla_stream_sync(d->st)) MFAIL(d, "first evaluation failed");
    } else if (nla_memcpy_h2d(d->d_P, x, xbytes, d->st) || mlsl_eval_rows(d, d->d_P, 1, d->d_F, d->st) ||
               nla_memcpy_d2h(d->F, d->d_F, sizeof(double), d->st) || nla_stream_sync(d->st)) MFAIL(d, "first evaluation failed");
    ++*d->stop->nevals_p;
    d->minimized[0] = 0; d->cpd[0] = HUGE_VAL; d->cld[0] = HUGE_VAL;          /* pts_insert of a fresh point */
    ord_insert(d->ord, d->npts, d->F, 0);
    ++d->npts;
    if (d->F[0] != d->F[0]) d->ord_has_nan = 1;
    if (mlsl_agree(d)) return -1;
    d->ret = mlsl_stop_after_sample(d, d->F[0]);
    return 0;
}

/* ---- sampling phase (mlsl.c:349-374) ---- */

/* the sampling phase's distance pass (find_closest_pt + pts_update_newpt, find_closest_lm) for the N new points in rows old .. old + N - 1:
 * everything it needs is on the device once the sampling kernel has run — the points, their f, the old points' closest_pt_d and flags
 * (uploaded here: the new rows' entries are set before) — so with a device objective on one rank it is ENQUEUED RIGHT BEHIND THE
 * SAMPLING KERNEL and runs while the host walks the N values (counts, stop tests, the order array: 0.3 ms per iteration that used to
 * stand between the sampling kernel and the distance kernel, profiles/r05_mlsl_timeline.txt).  A run that stops inside that walk
 * leaves; what the pass wrote is not looked at again.  Allocation first: nothing is enqueued before the scratch is large enough. */
static int mlsl_enqueue_distances(mlsl_dev *d, size_t old)
{
    const int na = d->N, nb = (int) (old + (size_t) d->N);
    const int per = (na + d->world - 1) / d->world;
    const int r0 = per * d->rank < na ? per * d->rank : na;
    const int mine = na - r0 < per ? na - r0 : per;
    if (need_D(d, (size_t) na * (size_t) nb) || (d->nlms && need_D(d, (size_t) na * d->nlms))) return -1;
    if (nla_memcpy_h2d(d->d_cpd, d->cpd, sizeof(double) * (size_t) nb, d->st) ||
        nla_memcpy_h2d(d->d_min, d->minimized, sizeof(int32_t) * (size_t) nb, d->st) ||
        mlsl_closest_pt_pass(d, d->st, old, r0, mine, d->d_D, d->d_cpd, d->d_min) ||
        nla_memcpy_d2h(d->cpd, d->d_cpd, sizeof(double) * (size_t) nb, d->st) ||
        mlsl_closest_lm_pass(d, d->st, old, r0, mine, 0, d->nlms, d->d_D, d->d_tmp, d->cld + old + r0)) MFAIL(d, "distance pass failed");
    return 0;
}

/* the samples were made beside the last local phase (mlsl_enqueue_ahead): nothing to launch for them.  What is left of the distance
 * pass: the new rows against the minima found since (this stream's work waits for the rows); then the values and the closest-point
 * minima are merged by `min` */
static int mlsl_take_ahead(mlsl_dev *d, size_t old)
{
    const size_t l0 = d->ahead_nlms, lc = d->nlms - d->ahead_nlms;
    size_t j;
    if (nla_stream_wait_event(d->st, d->ev_ahead)) MFAIL(d, "sampling failed");
    if (lc && (need_D(d, (size_t) d->N * lc) ||
               mlsl_closest_lm_pass(d, d->st, old, 0, d->N, l0, lc, d->d_D, d->d_tmp, d->cld + old))) MFAIL(d, "distance pass failed");
    if (nla_event_sync(d->ev_ahead)) MFAIL(d, "sampling failed");
    memcpy(d->Fnew, d->Fnew2, sizeof(double) * (size_t) d->N);
    if (d->stats) ++d->stats->mlsl_sampled_ahead;
    for (j = 0; j < old + (size_t) d->N; ++j) if (d->h_cpd2[j] < d->cpd[j]) d->cpd[j] = d->h_cpd2[j];
    return 0;
}

/* the host's walk over the N values in the reference's order (mlsl.c:360-368): a host objective is called here; counts, trace, the stop
 * tests after every sample; then the ordered insertion of the rows walked and the stream accounting.  Returns the samples used. */
static size_t mlsl_walk_samples(mlsl_dev *d, size_t old)
{
    double *Fnew = d->Fnew;
    size_t used = 0;
    int i;
    for (i = 0; i < d->N && d->ret == NLOPT_SUCCESS; ++i) {
        if (d->host) Fnew[i] = d->f((unsigned) d->n, d->h_rows + (size_t) i * (size_t) d->ld, NULL, d->f_data);   /* mlsl.c:360 */
        d->F[old + (size_t) i] = Fnew[i];
        ++*d->stop->nevals_p;
        if (d->stats) ++d->stats->evals_trial;
        ++d->npts;                             /* (entries initialised in front of the walk; ord_insert_run follows) */
        used = (size_t) i + 1;
        mlsl_trace(d->opt, Fnew[i], old + (size_t) i, 3, 0);
        d->ret = mlsl_stop_after_sample(d, Fnew[i]);
    }
    ord_insert_run(d->ord, old, d->F, old, used, d->ord_has_nan);
    for (i = 0; i < (int) used && !d->ord_has_nan; ++i) if (d->F[old + (size_t) i] != d->F[old + (size_t) i]) d->ord_has_nan = 1;
    if (d->d_V) d->sobol_next += (uint32_t) used;
    else d->words_used += 2ULL * (uint64_t) d->n * (uint64_t) used;
    return used;
}

static int mlsl_sampling_phase(mlsl_dev *d, double t0)
{
    const size_t old = d->npts;
    size_t used;
    int i, dist_enqueued = 0, ahead_hit;
    if (grow_pts(d, old + (size_t) d->N)) return -1;
    ahead_hit = d->ahead_valid && d->ahead_old == old && (d->d_V ? d->ahead_sobol == d->sobol_next : d->ahead_words == d->words_used);
    d->ahead_valid = 0;
    if (!ahead_hit) {
        if (d->d_V) {
            if ((uint64_t) d->sobol_next + (uint64_t) d->N >= 4294967295ULL) MFAIL(d, "Sobol sequence exhausted (2^32-1 points)");
        } else {
            if (d->prefetched_at != d->words_used &&
                nla_mtstream_fill(d->mts, d->words_used, 2ULL * (uint64_t) d->n * (uint64_t) d->N, d->d_words)) MFAIL(d, "MT stream fill failed");
            if (d->rs != d->st && nla_stream_sync(d->rs)) MFAIL(d, "MT stream fill failed");   /* the words are there */
        }
        if (mlsl_sample_rows(d, d->st, old, !d->host)) MFAIL(d, "sampling failed");
    }
    /* the new rows' closest-distance entries and flags start as "none yet" (what pts_insert does per point; here for all N at once so
     * that the distance pass can be enqueued before the host looks at a single value) */
    for (i = 0; i < d->N; ++i) { d->minimized[old + (size_t) i] = 0; d->cpd[old + (size_t) i] = HUGE_VAL; d->cld[old + (size_t) i] = HUGE_VAL; }
    if (ahead_hit) {
        if (mlsl_take_ahead(d, old)) return -1;
        dist_enqueued = 1;                                                     /* (everything is enqueued or done) */
    } else {
        if (d->host ? nla_memcpy_d2h(d->h_rows, d->d_P + old * (size_t) d->ld, sizeof(double) * (size_t) d->N * (size_t) d->ld, d->st)
                    : nla_memcpy_d2h(d->Fnew, d->d_F + old, sizeof(double) * (size_t) d->N, d->st)) MFAIL(d, "sampling failed");
        if (!d->host && d->world == 1) {
            /* wait for the values only (an event behind their copy, recorded BEFORE the distance pass goes out and synchronised
             * after it), with the distance pass already behind them on the stream */
            if (nla_event_record(d->ev_samples, d->st)) MFAIL(d, "sampling failed");
            if (mlsl_enqueue_distances(d, old)) return -1;
            dist_enqueued = 1;
            if (nla_event_sync(d->ev_samples)) MFAIL(d, "sampling failed");
        } else if (nla_stream_sync(d->st)) MFAIL(d, "sampling failed");
    }
    used = mlsl_walk_samples(d, old);
    if (d->host && (nla_memcpy_h2d(d->d_F + old, d->Fnew, sizeof(double) * used, d->st) || nla_stream_sync(d->st))) MFAIL(d, "sampling failed");
    if (d->ret != NLOPT_SUCCESS) return 0;
    /* the sampling kernel has read the words (synchronised above): the next iteration's can be generated.  NOT here (round 5,
     * profiles/r05_mlsl_timeline.txt): enqueued now, the jump-ahead kernel — 33 k workgroups, 0.55 ms, once or twice per iteration —
     * and the generator had the device to themselves and the distance pass queued up behind them, 0.9-1.8 ms of every iteration.
     * They go out right in front of the local searches' launch instead (mlsl_prefetch_now), on a background-priority stream: the
     * searches' 300 workgroups leave most of every compute unit free for 6 ms */
    d->prefetch_due = d->prefetch && !d->d_V;
    d->ahead_due = d->ahead;
    if (!dist_enqueued && mlsl_enqueue_distances(d, old)) return -1;
    if (nla_stream_sync(d->st)) MFAIL(d, "distance pass failed");
    if (ahead_hit && d->ahead_nlms)                                            /* closest_lm_d: the minima known when the rows were made | those found since */
        for (i = 0; i < d->N; ++i) if (d->h_cld2[i] < d->cld[old + (size_t) i]) d->cld[old + (size_t) i] = d->h_cld2[i];
    if (d->world > 1 && (min_over_ranks(d, d->cpd, d->npts) || (d->nlms && min_over_ranks(d, d->cld + old, (size_t) d->N))))
        MFAIL(d, "all-gather of the distance minima failed: %s", nlopt_amd_comm_error(d->comm));
    if (d->stats) d->stats->t_eval_s += nla_seconds() - t0;
    return 0;
}

/* ---- local phase (mlsl.c:377-428) ---- */

/* the walk of one iteration over the best ceil(gamma |pts|) points in `ord`, a batch of candidates at a time */
typedef struct {
    double R;                       /* the critical distance of this iteration (mlsl.c:377-379) */
    size_t idx; int remaining;      /* the walk: next position in ord, nodes left to visit */
    size_t scan; int rem;           /* the same behind the last node scanned for the current batch */
    int nb, per, mine;              /* the batch: candidates, slots per rank (gathered rows: per x world), searches of this rank */
    int pairs_enqueued;             /* the minimisers' distances went out behind the searches' kernel */
    int nacc; size_t nlms0;         /* minima the commit walk accepted, and where in the minimum set they start */
} mlsl_walk;

/* the next candidates that are potential minimisers right now (is_potential_minimizer, mlsl.c:196-221; the bound test follows on
 * the device) */
static void mlsl_select_candidates(mlsl_dev *d, mlsl_walk *w)
{
    const double R = w->R;
    w->nb = 0; w->scan = w->idx; w->rem = w->remaining;
    while (w->scan < d->npts && w->rem > 0 && w->nb < d->bmax) {
        const size_t r = d->ord[w->scan];
        ++w->scan; --w->rem;
        if (d->minimized[r] || d->cpd[r] <= R * R || d->cld[r] <= (dlm * R) * (dlm * R)) continue;
        d->cand[w->nb++] = w->scan - 1;
    }
}

/* the host search of the batch's one candidate (mlsl.c:400-407): through the library's own nlopt_optimize, its calls counted one by one */
static int mlsl_host_search(mlsl_dev *d, int mine)
{
    nla_lbfgs_result *res = d->res;
    const nla_stopping *stop = d->stop;
    const size_t xbytes = sizeof(double) * (size_t) d->n;
    memset(&res[0], 0, sizeof res[0]);
    if (mine > 0) {
        const double t = nla_seconds();
        double lf = HUGE_VAL;
        nlopt_result lret;
        if (nla_memcpy_d2h(d->cob_x, d->d_LX, xbytes, d->st) || nla_stream_sync(d->st)) MFAIL(d, "gather failed");
        lret = nla_optimize_limited(d->local_opt, d->cob_x, &lf, stop->maxeval - *stop->nevals_p, stop->maxtime - (t - stop->start));
        if (nla_memcpy_h2d(d->d_LX, d->cob_x, xbytes, d->st) || nla_stream_sync(d->st)) MFAIL(d, "minimum store failed");
        res[0].ret = (int) lret; res[0].f = lf;
        res[0].nevals = 0; res[0].iterm = 0;                                   /* the calls were counted one by one (mlsl_counted_f) */
    }
    return 0;
}

/* the batched searches of this rank's share on the device, and the all-gather of the minimisers and their results */
static int mlsl_device_searches(mlsl_dev *d, mlsl_walk *w)
{
    const int nb = w->nb, per = w->per, mine = w->mine;
    mlsl_pairs_job job;
    int c;
    if (!d->host && d->world == 1 && mine > 0) {
        /* one rank, device objective: the minimisers' distances go out right behind the searches' kernel (they need nothing the
         * host decides), instead of after the host has woken up, copied the results and come back: 0.2 ms per iteration.
         * (Allocation first: need_D in front of nla_local_ctx_after_launch) */
        job.d = d; job.nb = nb; job.na = (size_t) per; job.ctx_X = nla_local_ctx_X(d->lb);
        job.lx_bytes = sizeof(double) * (size_t) per * (size_t) d->ld;
        if (need_D(d, (size_t) per * d->npts)) return -1;
        for (c = 0; c < nb; ++c) d->h_gi[c] = (int64_t) mlsl_gi(c, d->world, per);
        nla_local_ctx_after_launch(d->lb, mlsl_enqueue_pairs, &job);
        w->pairs_enqueued = 1;
    }
    /* the prefetch and the sampling phase ahead go out directly in front of the launch, behind everything that may allocate (freeing
     * device memory waits for every stream, the gate included); gate_need is non-zero only around this call */
    d->gate_need = 0;
    if (d->ahead && mine > 0 && (d->gate_counter = nla_local_ctx_finished_counter(d->lb, &d->gate_from))) d->gate_need = (mine * NLA_MLSL_GATE_PCT + 99) / 100;
    c = mlsl_prefetch_now(d);
    d->gate_need = 0;
    if (c) return -1;
    if (mine > 0 && nla_local_ctx_run(d->lb, mine, &d->prm, d->res_mine, &d->lstop, NULL)) MFAIL(d, "local-search batch failed");
    if ((!w->pairs_enqueued && nla_comm_allgather_dev(d->comm, nla_local_ctx_X(d->lb), d->d_LX, sizeof(double) * (size_t) per * (size_t) d->ld, d->st)) ||
        nla_comm_allgather_host(d->comm, d->res_mine, d->res, sizeof *d->res * (size_t) per, d->st))
        MFAIL(d, "all-gather of the local minima failed: %s", nlopt_amd_comm_error(d->comm));
    return 0;
}

/* start points of this rank's share into the batch (one gather launch), and the bound test of every candidate (is_potential_minimizer,
 * mlsl.c:211-218) on the device: only the flags come back; then the local searches of this rank's share, the all-gather of the
 * minimisers, and their distances to every point.  d->ret != NLOPT_SUCCESS afterwards: the run stopped in front of a host search. */
static int mlsl_launch_batch(mlsl_dev *d, mlsl_walk *w)
{
    const int nb = w->nb, bmax = d->bmax;
    const int per = w->per = (nb + d->world - 1) / d->world;
    int c, mine = 0;
    w->pairs_enqueued = 0;
    for (c = 0; c < nb; ++c) d->h_idx[c] = (int64_t) d->ord[d->cand[c]];
    for (c = d->rank; c < nb; c += d->world, ++mine) d->h_idx[bmax + mine] = (int64_t) d->ord[d->cand[c]];
    if (nla_memcpy_h2d(d->d_idx, d->h_idx, sizeof(int64_t) * (size_t) (bmax + mine), d->st) ||
        nla_k_mlsl_gather_rows(d->n, d->ld, d->d_P, d->d_idx + bmax, mine, d->local == MLSL_HOST_SEARCH ? d->d_LX : nla_local_ctx_X(d->lb), d->st) ||
        nla_k_mlsl_near_bound(d->n, d->ld, d->d_P, d->d_idx, nb, d->d_lb, d->d_ub, dbound * w->R, d->d_flags, d->st) ||
        nla_memcpy_d2h(d->h_flags, d->d_flags, sizeof(int32_t) * (size_t) nb, d->st)) MFAIL(d, "gather failed");
    if (d->host && d->world == 1) {
        /* a host objective sees its calls: the tests the reference makes in front of a search (mlsl.c:390-399) are made
         * here, before the search's first callback, not at commit time */
        if (nla_stream_sync(d->st)) MFAIL(d, "gather failed");
        if (d->h_flags[0]) mine = 0;                                           /* too close to a bound: not started */
        else d->ret = mlsl_stop_before_host_search(d);
        if (d->ret != NLOPT_SUCCESS) return 0;
    }
    w->mine = mine;
    d->prm.maxeval = mlsl_eval_limit(d);
    if (d->local == MLSL_HOST_SEARCH ? mlsl_host_search(d, mine) : mlsl_device_searches(d, w)) return -1;
    {
        /* the distances of the batch's minimisers to every point stay on the device (na x npts: 12 MB at config 4); the commit walk
         * only needs those to the batch's OWN start points (whether an earlier commit of the batch disqualified a later
         * candidate, mlsl.c:180-194 seen from :196-221) — nb x nb values — and pts_update_newlm for all the other points is an
         * order-independent min that one launch computes once the accepted set is known */
        const size_t na = (size_t) per * (size_t) d->world;
        if (need_D(d, na * d->npts)) return -1;
        if (!w->pairs_enqueued) {
            mlsl_pairs_job job;
            for (c = 0; c < nb; ++c) d->h_gi[c] = (int64_t) mlsl_gi(c, d->world, per);
            job.d = d; job.nb = nb; job.na = na; job.ctx_X = NULL; job.lx_bytes = 0;
            if (mlsl_enqueue_pairs(&job)) MFAIL(d, "distance pass failed");
        }
        if (nla_stream_sync(d->st)) MFAIL(d, "distance pass failed");
        for (c = 0; c < (int) na; ++c) d->h_lfall[c] = HUGE_VAL;
        for (c = 0; c < nb; ++c) d->lf_cand[c] = HUGE_VAL;
    }
    return 0;
}

/* the limit binds differently than assumed: redo the one search of candidate c (start row r, gathered row g) alone with the exact
 * limit (every rank does, identically; the gathered rows of the other candidates are untouched) */
static int mlsl_rerun_search(mlsl_dev *d, const mlsl_walk *w, int c, size_t r, size_t g, int eff)
{
    const size_t xbytes = sizeof(double) * (size_t) d->n;
    const int nb = w->nb;
    nla_lbfgs_params p1 = d->prm;
    nla_lbfgs_result r1;
    int cp;
    p1.maxeval = eff;
    if (nla_memcpy_d2d(nla_local_ctx_X(d->lb), d->d_P + r * (size_t) d->ld, xbytes, d->st) ||
        nla_local_ctx_run(d->lb, 1, &p1, &r1, &d->lstop, NULL) ||
        nla_memcpy_d2d(d->d_LX + g * (size_t) d->ld, nla_local_ctx_X(d->lb), xbytes, d->st) ||
        nla_k_mlsl_dist2(d->n, d->ld, d->d_LX + g * (size_t) d->ld, 1, d->d_P, (int) d->npts, d->d_D + g * d->npts, d->st) ||
        nla_memcpy_d2h(d->h_D, d->d_D + g * d->npts, sizeof(double) * d->npts, d->st) || nla_stream_sync(d->st)) MFAIL(d, "local-search rerun failed");
    for (cp = 0; cp < nb; ++cp) d->h_S[(size_t) cp * (size_t) nb + (size_t) c] = d->h_D[d->ord[d->cand[cp]]];     /* this minimiser moved: its distances to the batch's start points */
    d->res[g] = r1;
    return 0;
}

/* commit the batch in walk order (mlsl.c:385-425 for each candidate, as the serial order would see it) */
static int mlsl_commit_batch(mlsl_dev *d, mlsl_walk *w)
{
    nlopt_amd_stats *st = d->stats;
    nla_stopping *stop = d->stop;
    nla_lbfgs_result *res = d->res;
    const size_t *cand = d->cand;
    const double R = w->R;
    const int nb = w->nb, bmax = d->bmax, use_mma = d->local == MLSL_MMA;
    const int tests_at_commit = !(d->host && d->world == 1);                   /* (else: made in front of the search, mlsl_launch_batch) */
    int c;
    if (grow_lms(d, d->nlms + (size_t) nb)) return -1;
    w->nacc = 0; w->nlms0 = d->nlms;
    for (c = 0; c < nb && d->ret == NLOPT_SUCCESS; ++c) {
        const size_t r = d->ord[cand[c]];
        double lf, cl = d->cld[r];
        int calls, pot, cp, eff;
        const size_t g = mlsl_gi(c, d->world, w->per);
        /* closest_lm_d of this start as the serial order would see it now: the minima committed earlier in this batch count
         * (pts_update_newlm, mlsl.c:180-194: those with smaller f than the point's, if closer) */
        /* (h_S[c][cp] = distance of start c to minimiser cp: transposed on the device.  nb^2 / 2 questions per batch — 46 k at config 4:
         * with the gathered-row index of cp, a division and a remainder, inside the loop they were the better part of the 0.6 ms the
         * device waited for this walk — hence the hoisted pointers: nothing is read through `d` in here) */
        {
            const double Fr = d->F[r], *Sc = d->h_S + (size_t) c * (size_t) nb, *lfc = d->lf_cand;
            for (cp = 0; cp < c; ++cp)
                if (lfc[cp] < Fr && Sc[cp] < cl) cl = Sc[cp];
        }
        pot = !(cl <= (dlm * R) * (dlm * R));
        /* nodes between the previous candidate and this one were visited and skipped */
        w->remaining -= (int) (cand[c] + 1 - w->idx);
        w->idx = cand[c] + 1;
        if (pot && d->h_flags[c]) pot = 0;                                     /* too close to a bound (mlsl.c:211-218) */
        if (!pot) continue;
        if (tests_at_commit) {                                                 /* mlsl.c:391-399, on the agreed view */
            if (nla_stop_forced(d->sp)) { d->ret = NLOPT_FORCED_STOP; break; }
            if (nla_stop_evals(stop)) { d->ret = NLOPT_MAXEVAL_REACHED; break; }
            if (nla_stop_time(d->sp)) { d->ret = NLOPT_MAXTIME_REACHED; break; }
        }
        /* did this search run under the evaluation limit it would have had in the serial order? */
        eff = mlsl_eval_limit(d);
        if (eff > 0 && eff != d->prm.maxeval && res[g].nevals >= eff && mlsl_rerun_search(d, w, c, r, g, eff)) return -1;
        calls = use_mma ? res[g].iterm : res[g].nevals;                        /* objective calls the search made (MMA: iterm) */
        *stop->nevals_p += calls;                                              /* fcount, mlsl.c:246-251 */
        if (st) { st->evals_mutation += (uint64_t) calls; ++st->accepted; }
        d->minimized[r] = 1;
        mlsl_trace(d->opt, res[g].f, r, 4, calls);
        if (res[g].ret < 0) { d->ret = (nlopt_result) res[g].ret; d->search_failed = 1; return 0; }
        lf = res[g].f;
        /* the minimum joins the device-side set; stream-ordered, no synchronisation per minimum (room for the whole
         * batch was made before the walk; res[] stays valid until the batch's closing synchronisation) */
        d->h_idx[bmax + BATCH_MAX + w->nacc] = (int64_t) g;
        d->h_lf[w->nacc] = lf;
        d->h_lfall[g] = lf;
        d->lf_cand[c] = lf;
        ++w->nacc;
        d->LF[d->nlms] = lf;
        ord_insert(d->lord, d->nlms, d->LF, d->nlms);
        ++d->nlms;
        d->ret = mlsl_stop_after_search(d, lf);
        /* (pts_update_newlm for this minimum: with the batch's other accepted minima, in one launch — mlsl_publish_minima.  A minimum
         * whose commit ends the run updated nothing in the reference either — the stop tests come first, mlsl.c:417-425 — so it is left out.) */
        if (d->ret != NLOPT_SUCCESS) { d->h_lfall[g] = HUGE_VAL; d->lf_cand[c] = HUGE_VAL; }
    }
    return 0;
}

/* the batch's accepted minima reach the points and the device-side set */
static int mlsl_publish_minima(mlsl_dev *d, const mlsl_walk *w)
{
    const int nacc = w->nacc, rows = w->per * d->world, bmax = d->bmax;
    /* pts_update_newlm (mlsl.c:180-194) for every accepted minimum of the batch at once: closest_lm_d[k] = min over the accepted
     * minima with smaller f than point k of their distance to k — a min, so the order of the commits does not matter.  (The
     * reference skips minimised points; their closest_lm_d is never read again, mlsl.c:200, so no flag is consulted here.) */
    if (nacc > 0 && (nla_memcpy_h2d(d->d_lfall, d->h_lfall, sizeof(double) * (size_t) rows, d->st) ||
                     nla_memcpy_h2d(d->d_cpd, d->cld, sizeof(double) * d->npts, d->st) ||
                     nla_k_mlsl_colmin(d->d_D, (int) d->npts, rows, (int) d->npts, d->d_lfall, d->d_F, NULL, d->d_cpd, d->st) ||
                     nla_memcpy_d2h(d->cld, d->d_cpd, sizeof(double) * d->npts, d->st))) MFAIL(d, "closest-minimum update failed");
    /* the batch's accepted minima join the device-side set in acceptance order: one gather launch */
    if (nacc > 0 && (nla_memcpy_h2d(d->d_idx + bmax + BATCH_MAX, d->h_idx + bmax + BATCH_MAX, sizeof(int64_t) * (size_t) nacc, d->st) ||
                     nla_k_mlsl_gather_rows(d->n, d->ld, d->d_LX, d->d_idx + bmax + BATCH_MAX, nacc, d->d_LM + w->nlms0 * (size_t) d->ld, d->st) ||
                     nla_memcpy_h2d(d->d_LF + w->nlms0, d->h_lf, sizeof(double) * (size_t) nacc, d->st))) MFAIL(d, "minimum store failed");
    if (nla_stream_sync(d->st)) MFAIL(d, "minimum store failed");
    return 0;
}

static int mlsl_local_phase(mlsl_dev *d)
{
    const double t0 = nla_seconds();
    mlsl_walk w;
    w.R = d->R_prefactor * pow(log((double) d->npts) / d->npts, 1.0 / d->n);
    w.idx = 0;
    w.remaining = (int) (ceil(MLSL_GAMMA * d->npts) + 0.5);
    while (w.idx < d->npts && w.remaining > 0 && d->ret == NLOPT_SUCCESS) {
        mlsl_select_candidates(d, &w);
        if (w.nb == 0) { w.idx = w.scan; w.remaining = w.rem; break; }
        if (mlsl_agree(d) || mlsl_launch_batch(d, &w)) return -1;
        if (d->ret != NLOPT_SUCCESS) break;                                    /* stopped in front of a host search */
        if (mlsl_commit_batch(d, &w)) return -1;
        if (d->search_failed) return 0;                                        /* (the reference's goto done from inside the walk) */
        if (mlsl_publish_minima(d, &w)) return -1;
        if (d->ret == NLOPT_SUCCESS) {
            /* nodes scanned after the last candidate of the batch (none qualified) are visited too */
            w.remaining -= (int) (w.scan - w.idx);
            w.idx = w.scan;
        }
    }
    if (mlsl_prefetch_now(d)) return -1;                                       /* (an iteration without a local search) */
    if (d->stats) { d->stats->t_evolve_s += nla_seconds() - t0; ++d->stats->generations; }
    return 0;
}

nlopt_result nla_mlsl_minimize(nlopt_opt opt, int n, nlopt_func f, void *f_data, const double *lb, const double *ub, double *x,
                               double *minf, nla_stopping *stop, nlopt_opt local_opt, int Nsamples, int lds)
{
    mlsl_dev D;
    nlopt_result ret;

    memset(&D, 0, sizeof D);
    if ((ret = mlsl_check_args(&D, stop, local_opt, Nsamples)) != NLOPT_SUCCESS) return ret;
    if ((ret = mlsl_setup(&D, opt, n, f, f_data, lb, ub, stop, local_opt, lds)) != NLOPT_SUCCESS) { mfree(&D); return ret; }
    D.ret = NLOPT_SUCCESS;
    if (D.world > 1) {
        const int all = nla_comm_agree_same(D.comm, 1, nla_problem_fingerprint(lds ? NLOPT_G_MLSL_LDS : NLOPT_G_MLSL, n, D.N, D.obj + 100 * (int) local_opt->algorithm, lb, ub, x, stop) + nla_params_fingerprint(opt) + nla_params_fingerprint(local_opt));
        if (all < 0) { nla_stop_msg(stop, NLA_MSG_RANKS_DIFFER); D.ret = NLOPT_INVALID_ARGS; goto done; }
        if (all == 0) { nla_stop_msg(stop, "nlopt_amd: another rank could not set up its MLSL device state"); D.ret = NLOPT_FAILURE; goto done; }
    }
    if (mlsl_first_point(&D, x)) goto devfail;
    while (D.ret == NLOPT_SUCCESS) {
        double t0 = nla_seconds();
        mlsl_get_minf(&D);                                                     /* mlsl.c:347 */
        if (mlsl_agree(&D)) goto devfail;
        if (opt && opt->progress) { opt->progress(opt->progress_data, D.stats ? (long) D.stats->generations : 0, (long) *stop->nevals_p); t0 = nla_seconds(); }
        if (mlsl_sampling_phase(&D, t0) || (D.ret == NLOPT_SUCCESS && mlsl_local_phase(&D))) goto devfail;
    }
    if (!D.search_failed) mlsl_get_minf(&D);                                   /* mlsl.c:431 */
    if (D.best_f < HUGE_VAL) {
        const double *src = D.best_is_lm ? D.d_LM + D.best_row * (size_t) D.ld : D.d_P + D.best_row * (size_t) D.ld;
        *minf = D.best_f;
        if (nla_memcpy_d2h(x, src, sizeof(double) * (size_t) n, D.st) || nla_stream_sync(D.st)) { nla_stop_msg(stop, "device engine: result read-back failed"); D.ret = NLOPT_FAILURE; }
    }
    goto done;
devfail:                                   /* a phase failed with D.err set: the one place that reports it */
    nla_stop_msg(stop, "device engine: %s", D.err);
    D.ret = NLOPT_FAILURE;
done:
    if (D.stats) D.stats->mt_words = D.words_used;
    ret = D.ret;
    mfree(&D);
    return ret;
}
