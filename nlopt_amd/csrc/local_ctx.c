/* local_ctx.c — the batch context of the local optimisers (nla_local_ctx): device buffers for up to `cap` simultaneous searches by
 * LD_LBFGS (hip/lbfgs_kernels.hip), LD_MMA (hip/mma_kernels.hip) or LN_COBYLA (bound constraints only: hip/cobyla_kernels.hip,
 * cobyla_global.hip, cobyla_ext.hip; nonlinear constraints from a user's device blocks: cobyla_con.hip) or LN_NELDERMEAD / LN_SBPLX
 * (hip/nldrmd_kernels.hip, hip/sbplx_kernels.hip) or LD_TNEWTON and its three variants (hip/tnewton_kernels.hip), and the loop that runs them.  Its callers: a lone nlopt_optimize(LD_LBFGS | LD_MMA | LN_NELDERMEAD | LN_SBPLX) with count = 1
 * (nla_local_minimize_one below, behind lbfgs_driver.c / mma_driver.c / nldrmd_driver.c; tnewton_driver.c), MLSL's local phase with one workgroup or wavefront per start
 * (mlsl_driver.c), nlopt_amd_optimize_batch (batch_driver.c).  What differs between the algorithms is one entry of the table ALGS.
 *
 * Three kinds of objective (nla_evaluator):
 *   device    a compiled-in device objective (nlopt_amd_objective): evaluated inside the kernel, a whole search is
 *             one launch; the host only watches the clock / the force_stop flag while it waits and raises the
 *             kernel's abort flag (plis.c:263,273,371, pssubs.c:914);
 *   host      any other nlopt_func: the reference's callback contract (nlopt.h:60-62) — f is called on the caller's
 *             thread, one x at a time, in the reference's order.  The kernel runs as a coroutine (include/nlopt_amd.h
 *             "External evaluation"): every vector operation of the search stays on the device, only x travels to the
 *             host and f / gradient back, once per evaluation;
 *   user      a device objective supplied by the user as a code object (nlopt_amd_set_device_objective, userobj.c):
 *             the same coroutine, the evaluations of all waiting searches of a batch made by one launch of the user's
 *             kernel. */
#include "nla_internal.h"
#include "objfuncs.h"
#include <math.h>
#include <sched.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* what an algorithm is to the context: the sizes of its buffers, its launch, its share of the statistics */
typedef struct {
    size_t (*save)(int n);                                      /* bytes per search of the coroutine's saved state (nla_local_ext.save) */
    void (*sizes)(int kind, int n, int ld, int mf, int cap, size_t *work, size_t *iwork, size_t *hist);   /* doubles, ints, doubles; 0: none */
    int ext_grad;                                               /* external evaluation delivers gradients: EG has a row per search */
    int (*launch)(nla_local_ctx *c, int obj, int count, const nla_lbfgs_params *P, const nla_local_ext *ext);
    uint64_t bytes_per_col, bytes_per_eval;                     /* lbfgs_bytes of a result: n x (per_col x cols + per_eval x nevals) */
} local_alg;

/* the device buffers of a context, in bytes */
enum { B_X, B_RES, B_REQ, B_EX, B_EG, B_EF, B_LIST, B_SAVE, B_WORK, B_IWORK, B_HIST, B_EC, B_COUNT };

struct nla_local_ctx {
    int alg, n, ld, cap, mf, mos;
    const local_alg *a;
    nla_evaluator ev;
    nla_mma_params mma;            /* LD_MMA: the algorithm's own parameters (the stopping values come with each run) */
    const double *d_sigma_init;    /* LD_MMA, LN_COBYLA, LN_NELDERMEAD: initial step on the device, or NULL */
    void *st;
    const double *d_lb, *d_ub;
    void *d[B_COUNT];              /* the buffers of local_layout(), where it gives them a size; below and in `ext`: the same, typed */
    double *d_X, *d_work, *d_hist;
    int *d_iwork;
    nla_lbfgs_result *d_res;
    void *ev0, *ev1;
    nlopt_amd_stats *stats;        /* optional: device time / algorithmic bytes of the launches are added here */
    /* options of a run (nla_local_ctx_set_options) */
    int exact;
    double *d_xtol_abs, *d_x_weights;
    int32_t *h_abort;              /* pinned, device-visible: 0, 100 (maxtime) or -999 (forced stop) */
    /* external evaluation */
    nla_local_ext ext;
    nla_local_req *h_req;          /* pinned */
    double *h_x, *h_g, *h_f;       /* pinned: one point, one gradient, cap values */
    int32_t *h_list, *d_list;      /* user objective: indices of the waiting searches */
    double *d_ftrace; int64_t ftrace_cap;   /* optional per-evaluation f trace (nla_local_ctx_set_ftrace) */
    int (*after_launch)(void *); void *after_arg;   /* one-shot: called right behind the next run's kernel launch (nla_local_ctx_after_launch) */
    int32_t *d_done; int32_t done_expected;         /* optional (nla_local_ctx_finished_counter): searches ended so far, on the device / launched so far */
    /* LN_COBYLA: batches too small to fill the device go through the host algorithm (cobyla_small_batch_on_host) */
    int cob_min_batch;
    double *h_lb, *h_ub, *h_dx, *h_xtol_abs, *h_rows;
    /* nlopt_amd_optimize_batch (batch_driver.c): a user kernel's waiting list built on the device (nla_local_ctx_set_device_list), the first
     * data row of this context's searches (nla_local_ctx_set_row0) */
    int dev_list;
    uint64_t *list_launches;       /* optional: steps whose list the device built */
    int32_t *d_nwait, *h_nwait;    /* the list's length: device word, pinned copy */
    int64_t row0;
    /* LN_COBYLA with nonlinear constraints (hip/cobyla_con.hip): the bound blocks in the reference's order and the first column of each
     * in a row of EC (B_EC: cap rows of ldc = mi + me values), the tolerances by column and the row map on the device */
    nla_usercon **con;
    int *con_col;
    int ncon, mi, me, ldc;
    double *d_con_tol;
    int32_t *d_rowmap;
    uint64_t *con_launches;
};

/* ---- the algorithms ---------------------------------------------------------------------------------------------------------------- */
#define SIZES(name) static void name(int kind, int n, int ld, int mf, int cap, size_t *work, size_t *iwork, size_t *hist)
static size_t lbfgs_save(int n) { (void) n; return nla_lbfgs_save_bytes(); }
SIZES(lbfgs_sizes)
{
    (void) kind; (void) n;
    *work = nla_lbfgs_work_doubles(ld, mf, cap); *iwork = (size_t) ld * (size_t) cap; *hist = nla_lbfgs_hist_doubles(ld, mf, cap);
}
static size_t mma_save(int n) { (void) n; return nla_mma_save_bytes(); }
SIZES(mma_sizes) { (void) kind; (void) n; (void) mf; (void) iwork; (void) hist; *work = nla_mma_work_doubles(ld, cap); }
/* LN_COBYLA, a compiled-in objective: the search's state in LDS while it fits there, its matrices in `work` beyond — where the device
 * layer has that kernel (the layout and the launch both ask here) */
static int cobyla_in_global_memory(int n) { return !nla_cobyla_fits(n) && nla_cobyla_global_serves(n); }
/* (a device layer without the coroutine has no saved state and no workspace for it: no such context is created there) */
static size_t cobyla_save(int n) { return nla_cobyla_save_bytes ? nla_cobyla_save_bytes(n) : 0; }
SIZES(cobyla_sizes)
{
    (void) mf; (void) hist;
    *work = kind == NLA_EVAL_USER ? (nla_cobyla_ext_work_doubles ? nla_cobyla_ext_work_doubles(n, cap) : 0)
          : cobyla_in_global_memory(n) ? nla_cobyla_global_work_doubles(n, cap) : nla_cobyla_work_doubles(n, ld, cap);   /* (the last a token) */
    *iwork = nla_cobyla_work_ints(n, cap);
}

static int lbfgs_launch(nla_local_ctx *c, int obj, int count, const nla_lbfgs_params *P, const nla_local_ext *ext)
{
    return nla_k_lbfgs_batch(obj, c->n, c->ld, c->mf, count, c->d_lb, c->d_ub, c->d_X, c->d_work, c->d_iwork, c->d_hist, P, c->d_res, ext, c->st);
}
/* the fields every algorithm's parameter record has, from launch()'s */
#define PARAMS_FROM(M, P) ((M).minf_max = (P)->minf_max, (M).ftol_rel = (P)->ftol_rel, (M).ftol_abs = (P)->ftol_abs, (M).xtol_rel = (P)->xtol_rel, \
                           (M).maxeval = (P)->maxeval, (M).exact = (P)->exact & 1, (M).sign = (P)->sign, (M).xtol_abs = (P)->xtol_abs,              \
                           (M).abort = (P)->abort, (M).done = (P)->done)
static int mma_launch(nla_local_ctx *c, int obj, int count, const nla_lbfgs_params *P, const nla_local_ext *ext)
{
    nla_mma_params M = c->mma;
    PARAMS_FROM(M, P);
    M.x_weights = P->x_weights; M.ftrace = P->ftrace; M.ftrace_cap = P->ftrace_cap;
    return nla_k_mma_batch(obj, c->n, c->ld, count, c->d_lb, c->d_ub, c->d_sigma_init, c->d_X, c->d_work, &M, c->d_res, ext, c->st);
}
static int cobyla_launch(nla_local_ctx *c, int obj, int count, const nla_lbfgs_params *P, const nla_local_ext *ext)
{
    nla_cobyla_params M;
    memset(&M, 0, sizeof M);
    PARAMS_FROM(M, P);
    if (c->ncon) return nla_k_cobyla_batch_ext_con(c->n, c->ld, count, c->d_lb, c->d_ub, c->d_sigma_init, c->d_X, c->d_work, &M, c->d_res, ext,
                                                   c->mi, c->me, c->ldc, (const double *) c->d[B_EC], c->d_con_tol, c->d_rowmap, c->st);
    if (ext) return nla_k_cobyla_batch_ext(c->n, c->ld, count, c->d_lb, c->d_ub, c->d_sigma_init, c->d_X, c->d_work, &M, c->d_res, ext, c->st);
    return (cobyla_in_global_memory(c->n) ? nla_k_cobyla_batch_global : nla_k_cobyla_batch)
               (obj, c->n, c->ld, count, c->d_lb, c->d_ub, c->d_sigma_init, c->d_X, c->d_work, c->d_iwork, &M, c->d_res, c->st);
}

/* LN_NELDERMEAD: the simplices in `work`, nothing else; the step (NULL: the default step of every start) as LD_MMA / LN_COBYLA take it */
static size_t nldrmd_save(int n) { return nla_nldrmd_save_bytes ? nla_nldrmd_save_bytes(n) : 0; }
SIZES(nldrmd_sizes) { (void) kind; (void) ld; (void) mf; (void) iwork; (void) hist; *work = nla_nldrmd_work_doubles ? nla_nldrmd_work_doubles(n, cap) : 0; }
static int nldrmd_launch(nla_local_ctx *c, int obj, int count, const nla_lbfgs_params *P, const nla_local_ext *ext)
{
    nla_nldrmd_params M;
    memset(&M, 0, sizeof M);
    PARAMS_FROM(M, P);
    M.x_weights = P->x_weights; M.ftrace = P->ftrace; M.ftrace_cap = P->ftrace_cap;
    return nla_k_nldrmd_batch(obj, c->n, c->ld, count, c->d_lb, c->d_ub, c->d_sigma_init, c->d_X, c->d_work, &M, c->d_res, ext, c->st);
}
/* LN_SBPLX: a search lives in LDS (`work` is a token); the parameters and the step are LN_NELDERMEAD's */
static size_t sbplx_save(int n) { return nla_sbplx_save_bytes ? nla_sbplx_save_bytes(n) : 0; }
SIZES(sbplx_sizes) { (void) kind; (void) ld; (void) mf; (void) iwork; (void) hist; *work = nla_sbplx_work_doubles ? nla_sbplx_work_doubles(n, cap) : 0; }
static int sbplx_launch(nla_local_ctx *c, int obj, int count, const nla_lbfgs_params *P, const nla_local_ext *ext)
{
    nla_sbplx_params M;
    memset(&M, 0, sizeof M);
    PARAMS_FROM(M, P);
    M.x_weights = P->x_weights; M.ftrace = P->ftrace; M.ftrace_cap = P->ftrace_cap;
    return nla_k_sbplx_batch(obj, c->n, c->ld, count, c->d_lb, c->d_ub, c->d_sigma_init, c->d_X, c->d_work, &M, c->d_res, ext, c->st);
}

/* LD_TNEWTON and its variants: ten vectors per search in `work`, the preconditioner's history (mf = 0 for the ids without one: none) */
static size_t tnewton_save(int n) { (void) n; return nla_tnewton_save_bytes ? nla_tnewton_save_bytes() : 0; }
SIZES(tnewton_sizes)
{
    (void) kind; (void) n;
    if (!nla_tnewton_has_launcher()) return;
    *work = nla_tnewton_work_doubles(ld, mf, cap); *iwork = (size_t) ld * (size_t) cap; *hist = nla_tnewton_hist_doubles(ld, mf, cap);
}
static int tnewton_launch(nla_local_ctx *c, int obj, int count, const nla_lbfgs_params *P, const nla_local_ext *ext)
{
    return nla_k_tnewton_batch(obj, c->n, c->ld, c->mf, c->mos, count, c->d_lb, c->d_ub, c->d_X, c->d_work, c->d_iwork, c->d_hist, P, c->d_res, ext, c->st);
}

static const local_alg ALGS[] = {
    /* (history columns streamed twice + the point written and read once per evaluation; mma_kernels.hip header; the point again) */
    [NLA_LOCAL_LBFGS]  = { lbfgs_save,  lbfgs_sizes,  1, lbfgs_launch,  32, 16 },
    [NLA_LOCAL_MMA]    = { mma_save,    mma_sizes,    1, mma_launch,    0,  64 },
    [NLA_LOCAL_COBYLA] = { cobyla_save, cobyla_sizes, 0, cobyla_launch, 0,  16 },   /* (never wants a gradient) */
    [NLA_LOCAL_NLDRMD] = { nldrmd_save, nldrmd_sizes, 0, nldrmd_launch, 0,  16 },   /* (never wants a gradient; the point, as LN_COBYLA counts it) */
    [NLA_LOCAL_SBPLX]  = { sbplx_save,  sbplx_sizes,  0, sbplx_launch,  0,  16 },   /* (the same) */
    /* per preconditioner column a dot and an axpy pass (16 n bytes; cols counts both recurrences of every application); per evaluation —
     * most are CG probes — the probe written and read, the quotient pass (3 vectors), the fused CG step (4 read, 2 written), <xs, xs>
     * and the direction update (3): 14 vectors of 8 n bytes */
    [NLA_LOCAL_TNEWTON] = { tnewton_save, tnewton_sizes, 1, tnewton_launch, 16, 112 },
};

/* THE layout: the size of every device buffer of a context for `cap` searches.  Allocation (nla_local_ctx_create) and the chunk size of
 * nlopt_amd_optimize_batch (nla_local_ctx_bytes_per_search) both read it.  mi, me: the values of a user's constraint blocks per search
 * (LN_COBYLA on a user's objective; 0, 0: none) — a row of EC each, and the save record and the slice sized for mi + 2 me more rows. */
static void local_layout(size_t b[B_COUNT], int alg, int kind, int n, int mf, int cap, int mi, int me)
{
    const local_alg *a = &ALGS[alg];
    const int ld = (n + 1) & ~1;
    const size_t rows = sizeof(double) * (size_t) ld * (size_t) cap;
    memset(b, 0, sizeof(size_t) * B_COUNT);
    b[B_X] = rows; b[B_RES] = sizeof(nla_lbfgs_result) * (size_t) cap;
    if (kind != NLA_EVAL_DEVICE) {
        b[B_REQ] = sizeof(nla_local_req) * (size_t) cap; b[B_EX] = rows; b[B_EG] = a->ext_grad ? rows : 0; b[B_EF] = sizeof(double) * (size_t) cap;
        b[B_LIST] = sizeof(int32_t) * (size_t) cap; b[B_SAVE] = a->save(n) * (size_t) cap;
    }
    a->sizes(kind, n, ld, mf, cap, &b[B_WORK], &b[B_IWORK], &b[B_HIST]);
    b[B_WORK] *= sizeof(double); b[B_IWORK] *= sizeof(int); b[B_HIST] *= sizeof(double);
    if (alg == NLA_LOCAL_COBYLA && kind == NLA_EVAL_USER && mi + me > 0 && nla_cobyla_con_has_launcher()) {
        b[B_EC] = sizeof(double) * (size_t) (mi + me) * (size_t) cap;
        b[B_SAVE] = nla_cobyla_con_save_bytes(n, mi + 2 * me) * (size_t) cap;
        b[B_WORK] = sizeof(double) * nla_cobyla_con_work_doubles(n, mi + 2 * me, cap);
    }
}
/* device memory one search takes in a context of algorithm alg (not in it: pinned host memory, the 8 doubles that stand for EG where no
 * gradient is delivered) */
size_t nla_local_ctx_bytes_per_search_con(int alg, const nla_evaluator *ev, int n, int mf, int mi, int me)
{
    size_t b[B_COUNT], sum = 0;
    int i;
    local_layout(b, alg, ev->kind, n, mf, 1, mi, me);
    for (i = 0; i < B_COUNT; ++i) sum += b[i];
    return sum;
}
size_t nla_local_ctx_bytes_per_search(int alg, const nla_evaluator *ev, int n, int mf) { return nla_local_ctx_bytes_per_search_con(alg, ev, n, mf, 0, 0); }

void nla_local_ctx_destroy(nla_local_ctx *c)
{
    int i;
    if (!c) return;
    for (i = 0; i < B_COUNT; ++i) nla_dev_free(c->d[i]);
    nla_dev_free(c->d_xtol_abs); nla_dev_free(c->d_x_weights);
    nla_dev_free(c->d_con_tol); nla_dev_free(c->d_rowmap); free(c->con); free(c->con_col);
    nla_dev_free(c->d_ftrace); nla_dev_free(c->d_nwait); nla_host_free(c->h_nwait);
    if (c->d_done) nla_dev_free_uncached(c->d_done);
    nla_host_free(c->h_abort); nla_host_free(c->h_req); nla_host_free(c->h_x); nla_host_free(c->h_g); nla_host_free(c->h_f);
    nla_host_free(c->h_list);
    free(c->h_lb); free(c->h_ub); free(c->h_dx); free(c->h_xtol_abs); free(c->h_rows);
    nla_event_destroy(c->ev0); nla_event_destroy(c->ev1);
    free(c);
}

/* ... the threshold can be set: 1 = every batch on the device, 0 / negative = the default above ("amd_cobyla_min_batch"); not for a user's
 * kernel, whose threshold stays 1 */
void nla_local_ctx_set_cobyla_min_batch(nla_local_ctx *c, int min_batch)
{
    if (c && c->alg == NLA_LOCAL_COBYLA && c->ev.kind == NLA_EVAL_DEVICE && min_batch > 0) c->cob_min_batch = min_batch;
}

/* the constraint blocks of *s into the context: the blocks and their columns, the tolerances and the row map (the reference's row order,
 * cobyla.c:106-119: row k < mi is -g_k; an equality block of b values gives b rows +h, then b rows -h) on the device.  0 or -1. */
static int con_setup(nla_local_ctx *c, const nla_local_spec *s)
{
    const int mc = s->mi + 2 * s->me;
    int32_t *map = (int32_t *) malloc(sizeof(int32_t) * (size_t) mc);
    int i, j, col = 0, row = 0, rc = -1;
    c->con = (nla_usercon **) malloc(sizeof *c->con * (size_t) s->ncon);
    c->con_col = (int *) malloc(sizeof(int) * (size_t) s->ncon);
    c->d_con_tol = (double *) nla_dev_malloc(sizeof(double) * (size_t) (s->mi + s->me));
    c->d_rowmap = (int32_t *) nla_dev_malloc(sizeof(int32_t) * (size_t) mc);
    if (!map || !c->con || !c->con_col || !c->d_con_tol || !c->d_rowmap) goto done;
    for (i = 0; i < s->ncon; ++i) {
        const int b = (int) nla_usercon_m(s->con[i]);
        c->con[i] = s->con[i]; c->con_col[i] = col;
        if (row + (i < s->ncon - s->ncon_eq ? b : 2 * b) > mc) goto done;          /* (the blocks do not add up to mi, me) */
        if (i < s->ncon - s->ncon_eq) for (j = 0; j < b; ++j) map[row++] = -(col + j + 1);
        else {
            for (j = 0; j < b; ++j) map[row++] = col + j;
            for (j = 0; j < b; ++j) map[row++] = -(col + j + 1);
        }
        col += b;
    }
    if (row != mc || col != s->mi + s->me) goto done;
    c->ncon = s->ncon; c->mi = s->mi; c->me = s->me; c->ldc = s->mi + s->me; c->con_launches = s->con_launches;
    rc = nla_memcpy_h2d(c->d_con_tol, s->con_tol, sizeof(double) * (size_t) c->ldc, c->st) || nla_memcpy_h2d(c->d_rowmap, map, sizeof(int32_t) * (size_t) mc, c->st) ||
         nla_stream_sync(c->st) ? -1 : 0;
done:
    free(map);
    return rc;
}

/* the context of *s (nla_internal.h); NULL: out of memory, or LN_COBYLA for a host callback or a dimension no device launcher serves, or
 * LN_NELDERMEAD / LN_SBPLX on a device layer without its launcher or at a dimension it does not serve, or LD_TNEWTON* without its launcher, or
 * constraint blocks for anything but LN_COBYLA on a user's objective at an (n, mc) the constrained launcher serves */
nla_local_ctx *nla_local_ctx_create(const nla_local_spec *s)
{
    const int kind = s->ev->kind;
    size_t b[B_COUNT];
    nla_local_ctx *c;
    int i;
    if (s->alg == NLA_LOCAL_COBYLA && !nla_cobyla_device_serves(kind, s->n)) return NULL;
    if (s->alg == NLA_LOCAL_NLDRMD && !nla_nldrmd_device_serves(s->n)) return NULL;
    if (s->alg == NLA_LOCAL_SBPLX && !nla_sbplx_device_serves(s->n)) return NULL;
    if (s->alg == NLA_LOCAL_TNEWTON && (!nla_tnewton_has_launcher() || s->mos < 0 || s->mos > 3 || (s->mos >= 2 ? s->mf < 1 : s->mf != 0))) return NULL;
    if (s->ncon > 0 && (s->alg != NLA_LOCAL_COBYLA || kind != NLA_EVAL_USER || !s->con || !s->con_tol || s->mi < 0 || s->me < 0 ||
                        !nla_cobyla_con_device_serves(s->n, s->mi + 2 * s->me))) return NULL;
    c = (nla_local_ctx *) calloc(1, sizeof *c);
    if (!c) return NULL;
    c->alg = s->alg; c->a = &ALGS[s->alg]; c->ev = *s->ev; c->n = s->n; c->ld = (s->n + 1) & ~1; c->cap = s->cap; c->mf = s->mf; c->mos = s->mos;
    if (s->mma) c->mma = *s->mma;
    c->d_sigma_init = s->d_step; c->d_lb = s->d_lb; c->d_ub = s->d_ub; c->st = s->stream;
    local_layout(b, s->alg, kind, s->n, s->mf, s->cap, s->ncon > 0 ? s->mi : 0, s->ncon > 0 ? s->me : 0);
    if (kind != NLA_EVAL_DEVICE && !b[B_EG]) b[B_EG] = sizeof(double) * 8;      /* (no gradient is ever delivered: a token) */
    for (i = 0; i < B_COUNT; ++i) if (b[i] && !(c->d[i] = nla_dev_malloc(b[i]))) goto fail;
    c->d_X = (double *) c->d[B_X]; c->d_res = (nla_lbfgs_result *) c->d[B_RES]; c->d_list = (int32_t *) c->d[B_LIST];
    c->d_work = (double *) c->d[B_WORK]; c->d_iwork = (int *) c->d[B_IWORK]; c->d_hist = (double *) c->d[B_HIST];
    c->ext.req = (nla_local_req *) c->d[B_REQ]; c->ext.EX = (double *) c->d[B_EX]; c->ext.EG = (double *) c->d[B_EG];
    c->ext.EF = (double *) c->d[B_EF]; c->ext.save = c->d[B_SAVE];
    c->h_abort = (int32_t *) nla_host_malloc(sizeof(int32_t));
    c->ev0 = nla_event_create(); c->ev1 = nla_event_create();
    if (!c->h_abort || !c->ev0 || !c->ev1) goto fail;
    *c->h_abort = 0;
    if (kind != NLA_EVAL_DEVICE) {
        c->h_req = (nla_local_req *) nla_host_malloc(sizeof(nla_local_req) * (size_t) c->cap);
        c->h_x = (double *) nla_host_malloc(sizeof(double) * (size_t) c->ld);
        c->h_g = (double *) nla_host_malloc(sizeof(double) * (size_t) c->ld);
        c->h_f = (double *) nla_host_malloc(sizeof(double) * (size_t) c->cap);
        c->h_list = (int32_t *) nla_host_malloc(sizeof(int32_t) * (size_t) c->cap);
        if (!c->h_req || !c->h_x || !c->h_g || !c->h_f || !c->h_list) goto fail;
    }
    if (s->ncon > 0 && con_setup(c, s)) goto fail;
    if (s->alg == NLA_LOCAL_COBYLA) {
        /* host copies of the box and the step for the host twin (cobyla_small_batch_on_host), and from how many searches on a batch
         * runs on the device */
        const size_t nb = sizeof(double) * (size_t) c->n;
        c->h_lb = (double *) malloc(nb); c->h_ub = (double *) malloc(nb);
        c->h_rows = (double *) malloc(sizeof(double) * (size_t) c->ld * (size_t) c->cap);
        if (c->d_sigma_init) c->h_dx = (double *) malloc(nb);
        if (!c->h_lb || !c->h_ub || !c->h_rows || (c->d_sigma_init && !c->h_dx) ||
            nla_memcpy_d2h(c->h_lb, c->d_lb, nb, c->st) || nla_memcpy_d2h(c->h_ub, c->d_ub, nb, c->st) ||
            (c->d_sigma_init && nla_memcpy_d2h(c->h_dx, c->d_sigma_init, nb, c->st)) || nla_stream_sync(c->st)) goto fail;
        /* One wavefront walks a search's serial chain 4 - 20 times slower than a host core (measured per evaluation of ONE search, device
         * against the reference on the same box, profiles/r06_cobyla_batched.txt: n = 8 21.7 us against 1.0, n = 16 40.6 against 4.2,
         * n = 32 133 against 26, n = 48 380 against 88) and hundreds of them run side by side (2048 searches: 56x / 104x one core at n = 8 / 16):
         * the device is the faster place from about that many concurrent searches on, the host below.  n > 51, the global-memory kernel
         * (profiles/r07_cobyla_global.txt, per iteration behind the initial simplex): n = 52 1.14 ms against 0.14, n = 64 2.17 against
         * 0.22, n = 128 16.1 against 2.5 — one search is 6 - 10 times a host core's time and up to 64 cost no more than one, so the
         * device is ahead from 7 (n = 128) to 10 (n = 64) searches on */
        c->cob_min_batch = c->n < 12 ? 24 : c->n < 24 ? 12 : nla_cobyla_fits(c->n) ? 6 : 10;
        /* A user's kernel has no host twin that is guaranteed to give its bits, and a run's result must not depend on how its searches happen
         * to be batched: every batch of such an objective, a lone search included, runs on the device */
        if (c->ev.kind == NLA_EVAL_USER) c->cob_min_batch = 1;
    }
    return c;
fail:
    nla_local_ctx_destroy(c);
    return NULL;
}
void nla_local_ctx_set_stats(nla_local_ctx *c, nlopt_amd_stats *stats) { if (c) c->stats = stats; }
/* work the caller wants on the context's stream RIGHT BEHIND the searches' kernel — enqueued before the host waits for the kernel, so that
 * it starts the moment the last search ends (MLSL: the minimisers' distances to the point set).  One-shot; device objectives only (a
 * run that goes through host evaluations calls it before it returns, with the searches finished).  A nonzero return fails the run. */
void nla_local_ctx_after_launch(nla_local_ctx *c, int (*fn)(void *), void *arg) { if (c) { c->after_launch = fn; c->after_arg = arg; } }
static int run_after_launch(nla_local_ctx *c)
{
    int (*fn)(void *) = c->after_launch;
    c->after_launch = NULL;
    return fn ? fn(c->after_arg) : 0;
}

/* device objectives: a counter on the device that every search of this context's launches adds 1 to when it ends (never reset).
 * nla_local_ctx_count_finished switches it on (0, or -1: no memory / searches that evaluate on the host); nla_local_ctx_finished_counter
 * returns it (NULL: not switched on) and in *from its value once everything launched so far has ended. */
int nla_local_ctx_count_finished(nla_local_ctx *c)
{
    if (!c || c->ev.kind != NLA_EVAL_DEVICE) return -1;
    if (c->d_done) return 0;
    c->d_done = (int32_t *) nla_dev_malloc_uncached(sizeof(int32_t));
    if (!c->d_done) return -1;
    if (nla_memset(c->d_done, 0, sizeof(int32_t), c->st) || nla_stream_sync(c->st)) { nla_dev_free_uncached(c->d_done); c->d_done = NULL; return -1; }
    c->done_expected = 0;
    return 0;
}
const int32_t *nla_local_ctx_finished_counter(nla_local_ctx *c, int32_t *from)
{
    if (!c || !c->d_done) return NULL;
    *from = c->done_expected;
    return c->d_done;
}
/* 1: from now on the waiting list of a user kernel's coroutine step is built by nla_k_local_waiting_list and the host reads back its
 * length only; 0: switched off, not a user kernel's context, or a device layer without the launcher — the host loop builds it */
int nla_local_ctx_set_device_list(nla_local_ctx *c, int on, uint64_t *launches)
{
    if (!c) return 0;
    c->dev_list = 0; c->list_launches = launches;
    if (!on || c->ev.kind != NLA_EVAL_USER || !nla_k_local_waiting_list) return 0;
    if (!c->d_nwait) c->d_nwait = (int32_t *) nla_dev_malloc(sizeof(int32_t));
    if (!c->h_nwait) c->h_nwait = (int32_t *) nla_host_malloc(sizeof(int32_t));
    if (!c->d_nwait || !c->h_nwait) return 0;
    return c->dev_list = 1;
}
void nla_local_ctx_set_row0(nla_local_ctx *c, int64_t row0) { if (c) c->row0 = row0; }
double *nla_local_ctx_X(nla_local_ctx *c) { return c->d_X; }

/* exact-order sums ("amd_exact_dot"), per-coordinate x tolerances and weights (host arrays of n or NULL; stop.c:98-120) */
int nla_local_ctx_set_options(nla_local_ctx *c, int exact, const double *xtol_abs, const double *x_weights)
{
    c->exact = exact;
    nla_dev_free(c->d_xtol_abs); nla_dev_free(c->d_x_weights);
    c->d_xtol_abs = c->d_x_weights = NULL;
    free(c->h_xtol_abs); c->h_xtol_abs = NULL;
    if (xtol_abs && c->alg == NLA_LOCAL_COBYLA) {
        c->h_xtol_abs = (double *) malloc(sizeof(double) * (size_t) c->n);
        if (!c->h_xtol_abs) return -1;
        memcpy(c->h_xtol_abs, xtol_abs, sizeof(double) * (size_t) c->n);
    }
    if (xtol_abs) {
        c->d_xtol_abs = (double *) nla_dev_malloc(sizeof(double) * (size_t) c->ld);
        if (!c->d_xtol_abs || nla_memcpy_h2d(c->d_xtol_abs, xtol_abs, sizeof(double) * (size_t) c->n, c->st)) return -1;
    }
    if (x_weights) {
        c->d_x_weights = (double *) nla_dev_malloc(sizeof(double) * (size_t) c->ld);
        if (!c->d_x_weights || nla_memcpy_h2d(c->d_x_weights, x_weights, sizeof(double) * (size_t) c->n, c->st)) return -1;
    }
    return nla_stream_sync(c->st);
}

/* record f of every evaluation of each search (cap per search); read back with nla_local_ctx_read_ftrace */
int nla_local_ctx_set_ftrace(nla_local_ctx *c, int64_t cap)
{
    nla_dev_free(c->d_ftrace);
    c->d_ftrace = NULL; c->ftrace_cap = 0;
    if (cap <= 0) return 0;
    c->d_ftrace = (double *) nla_dev_malloc(sizeof(double) * (size_t) cap * (size_t) c->cap);
    if (!c->d_ftrace) return -1;
    c->ftrace_cap = cap;
    return 0;
}
int nla_local_ctx_read_ftrace(nla_local_ctx *c, int inst, int64_t count, double *h_out)
{
    if (!c->d_ftrace || count > c->ftrace_cap) return -1;
    if (nla_memcpy_d2h(h_out, c->d_ftrace + (size_t) inst * (size_t) c->ftrace_cap, sizeof(double) * (size_t) count, c->st)) return -1;
    return nla_stream_sync(c->st);
}

/* one launch of the algorithm's kernel: the run's stopping values with what the context knows, in LD_LBFGS's record (it has every field;
 * the other launchers copy theirs out of it) */
static int launch(nla_local_ctx *c, int count, const nla_lbfgs_params *prm, const nla_local_ext *ext)
{
    nla_lbfgs_params P = *prm;
    P.exact = c->exact; P.sign = c->ev.sign; P.xtol_abs = c->d_xtol_abs; P.x_weights = c->d_x_weights; P.abort = c->h_abort;
    P.ftrace = c->d_ftrace; P.ftrace_cap = c->ftrace_cap; P.done = ext ? NULL : c->d_done;
    return c->a->launch(c, c->ev.kind == NLA_EVAL_DEVICE ? c->ev.obj : NLA_OBJ_EXTERNAL, count, &P, ext);
}

/* LN_COBYLA, a batch of fewer searches than the device needs to beat a host core (cob_min_batch): the rows come to the host, each search
 * runs through the library's own nlopt_optimize(LN_COBYLA) (cobyla_host.c: the reference's run evaluation by evaluation) on the
 * objective's host twin, the results go back to where the kernel would have left them.  In exact-order mode the twin's values ARE the
 * kernel's (same summation order, IEEE arithmetic), so where a batch runs changes nothing; in the default mode they differ by the
 * rounding of the tree sum. */
typedef struct { int obj; double sign; const nla_stopping *stop; nlopt_opt loc; int timed; } cob_host_obj;
static double cob_host_f(unsigned n, const double *x, double *g, void *p)
{
    cob_host_obj *o = (cob_host_obj *) p;
    (void) g;
    if (o->stop) {
        if (nla_stop_forced(o->stop)) nlopt_force_stop(o->loc);
        else if (nla_stop_time(o->stop)) { o->timed = 1; nlopt_force_stop(o->loc); }
    }
    return o->sign * nla_obj_eval_seq(o->obj, n, x, NULL);
}
static int cobyla_small_batch_on_host(nla_local_ctx *c, int count, const nla_lbfgs_params *prm, nla_lbfgs_result *h_res, const nla_stopping *stop)
{
    const size_t rows = sizeof(double) * (size_t) c->ld * (size_t) count;
    int rc, i;
    if ((rc = nla_memcpy_d2h(c->h_rows, c->d_X, rows, c->st)) || (rc = nla_stream_sync(c->st))) return rc;
    for (i = 0; i < count; ++i) {
        cob_host_obj o = { c->ev.obj & 0xff, (c->ev.sign == 0. ? 1. : c->ev.sign) * ((c->ev.obj & 0x100) ? -1. : 1.), stop, NULL, 0 };
        nlopt_opt loc = nlopt_create(NLOPT_LN_COBYLA, (unsigned) c->n);
        double minf = HUGE_VAL;
        if (!loc) return -1;
        o.loc = loc;
        nlopt_set_min_objective(loc, cob_host_f, &o);
        nlopt_set_lower_bounds(loc, c->h_lb); nlopt_set_upper_bounds(loc, c->h_ub);
        nlopt_set_stopval(loc, prm->minf_max); nlopt_set_ftol_rel(loc, prm->ftol_rel); nlopt_set_ftol_abs(loc, prm->ftol_abs); nlopt_set_xtol_rel(loc, prm->xtol_rel);
        if (c->h_xtol_abs) nlopt_set_xtol_abs(loc, c->h_xtol_abs);
        nlopt_set_maxeval(loc, prm->maxeval);
        if (c->h_dx) nlopt_set_initial_step(loc, c->h_dx);
        h_res[i].ret = nlopt_optimize(loc, c->h_rows + (size_t) i * (size_t) c->ld, &minf);
        if (o.timed && h_res[i].ret == NLOPT_FORCED_STOP) h_res[i].ret = NLOPT_MAXTIME_REACHED;
        h_res[i].f = minf; h_res[i].nevals = h_res[i].iterm = nlopt_get_numevals(loc); h_res[i].cols = 0;
        nlopt_destroy(loc);
    }
    if ((rc = nla_memcpy_h2d(c->d_X, c->h_rows, rows, c->st))) return rc;
    if ((rc = run_after_launch(c))) return rc;
    if ((rc = nla_stream_sync(c->st))) return rc;
    if (c->stats) c->stats->cobyla_host_searches += (uint64_t) count;
    return 0;
}

/* wait for the stream; meanwhile forward the caller's force_stop flag and maxtime to the kernel's abort flag */
static int wait_watching(nla_local_ctx *c, const nla_stopping *stop)
{
    int rc;
    if (!stop || (!stop->force_stop && stop->maxtime <= 0)) return nla_stream_sync(c->st);
    while ((rc = nla_stream_query(c->st)) == -1) {
        if (nla_stop_forced(stop)) *(volatile int32_t *) c->h_abort = -999;
        else if (nla_stop_time(stop)) *(volatile int32_t *) c->h_abort = 100;
        sched_yield();
    }
    return rc;
}

/* LN_COBYLA with constraint blocks, behind the objective's launch of a step: every block at ALL `count` rows of EX into its columns of EC
 * (the blocks' kernels take no list: the rows of finished searches are evaluated again and nobody reads them) */
static int eval_constraints(nla_local_ctx *c, int count, const double *EX)
{
    int i, rc;
    for (i = 0; i < c->ncon; ++i) {
        if ((rc = nla_usercon_eval_rows(c->con[i], c->n, c->ld, (int64_t) count, EX, c->ldc, (double *) c->d[B_EC] + c->con_col[i], c->st))) return rc;
        if (c->con_launches) ++*c->con_launches;
    }
    return 0;
}

/* run `count` searches from the rows already in ctx X; minimisers stay there, results come to the host.  stop (may be
 * NULL): the caller's force_stop flag and time limit, observed during the searches; live_nevals (may be NULL; host
 * objective only): incremented at every counted evaluation as the reference does (plis.c:261,391; mma.c:219,298). */
int nla_local_ctx_run(nla_local_ctx *c, int count, const nla_lbfgs_params *prm, nla_lbfgs_result *h_res, const nla_stopping *stop,
                      int *live_nevals)
{
    int rc, i;
    if (count > c->cap) return -1;
    if (c->alg == NLA_LOCAL_COBYLA && count < c->cob_min_batch) return cobyla_small_batch_on_host(c, count, prm, h_res, stop);
    *c->h_abort = 0;
    nla_event_record(c->ev0, c->st);
    if (c->ev.kind == NLA_EVAL_DEVICE) {
        if ((rc = launch(c, count, prm, NULL))) return rc;
        if (c->d_done) c->done_expected = (int32_t) ((uint32_t) c->done_expected + (uint32_t) count);
    } else {
        nla_local_ext E = c->ext;
        const size_t rowb = sizeof(double) * (size_t) c->n;
        if ((rc = nla_memset(E.req, 0, sizeof(nla_local_req) * (size_t) count, c->st))) return rc;
        /* (a search that ends before its first evaluation never writes its row of EX, and the blocks are evaluated at every row) */
        if (c->ncon && (rc = nla_memset(E.EX, 0, sizeof(double) * (size_t) c->ld * (size_t) count, c->st))) return rc;
        E.resume = 0;
        for (;;) {
            int waiting = 0;
            E.forced = stop ? nla_stop_forced(stop) : 0;
            E.timeout = stop ? nla_stop_time(stop) : 0;
            if ((rc = launch(c, count, prm, &E))) return rc;
            if (c->dev_list) {
                /* the list is built where the records are (hip/local_list.hip: the host loop's list entry for entry); one int32 comes back */
                if ((rc = nla_k_local_waiting_list(E.req, count, c->d_list, c->d_nwait, c->st))) return rc;
                if ((rc = nla_memcpy_d2h(c->h_nwait, c->d_nwait, sizeof(int32_t), c->st))) return rc;
                if ((rc = nla_stream_sync(c->st))) return rc;
                if (c->list_launches) ++*c->list_launches;
                if (*c->h_nwait <= 0) break;
                if ((rc = nla_userobj_evalgrad_list_rows(c->ev.user, c->n, c->ld, (int) *c->h_nwait, c->d_list, E.EX, E.EF, E.EG, c->ev.sign,
                                                         c->row0, count, c->st))) return rc;
                if (c->ncon && (rc = eval_constraints(c, count, E.EX))) return rc;
                E.resume = 1;
                continue;
            }
            if ((rc = nla_memcpy_d2h(c->h_req, E.req, sizeof(nla_local_req) * (size_t) count, c->st))) return rc;
            if ((rc = nla_stream_sync(c->st))) return rc;
            for (i = 0; i < count; ++i) waiting += c->h_req[i].state == 1;
            if (!waiting) break;
            if (c->ev.kind == NLA_EVAL_USER) {
                /* every waiting search is evaluated by one launch of the user's kernel; list entry i: search i wants its
                 * gradient, -(i+1): the value only */
                int m = 0;
                for (i = 0; i < count; ++i) if (c->h_req[i].state == 1) c->h_list[m++] = (c->h_req[i].want_grad & 1) ? i : -(i + 1);
                if ((rc = nla_memcpy_h2d(c->d_list, c->h_list, sizeof(int32_t) * (size_t) m, c->st))) return rc;
                if ((rc = nla_userobj_evalgrad_list_rows(c->ev.user, c->n, c->ld, m, c->d_list, E.EX, E.EF, E.EG, c->ev.sign, c->row0, count, c->st))) return rc;
                if (c->ncon && (rc = eval_constraints(c, count, E.EX))) return rc;
            } else {
                for (i = 0; i < count; ++i) {
                    const int want = c->h_req[i].want_grad;          /* bit 0: gradient wanted; bit 1: LD_MMA's uncounted call (mma.c:337-339) */
                    if (c->h_req[i].state != 1) continue;
                    if ((rc = nla_memcpy_d2h(c->h_x, E.EX + (size_t) i * c->ld, rowb, c->st)) || (rc = nla_stream_sync(c->st))) return rc;
                    c->h_f[i] = c->ev.f((unsigned) c->n, c->h_x, (want & 1) ? c->h_g : NULL, c->ev.f_data);
                    if (live_nevals && !(want & 2)) ++*live_nevals;
                    if ((rc = nla_memcpy_h2d(E.EF + i, c->h_f + i, sizeof(double), c->st))) return rc;
                    if ((want & 1) && (rc = nla_memcpy_h2d(E.EG + (size_t) i * c->ld, c->h_g, rowb, c->st))) return rc;
                    if ((rc = nla_stream_sync(c->st))) return rc;         /* h_g is reused by the next evaluation */
                }
            }
            E.resume = 1;
        }
    }
    nla_event_record(c->ev1, c->st);
    if ((rc = run_after_launch(c))) return rc;
    /* a kernel that runs the whole search: watch first, copy afterwards — a device-to-host copy into pageable memory (the caller's result
     * record may live on its stack) does not return before the kernel has finished, and nobody would raise the abort flag meanwhile */
    if (c->ev.kind == NLA_EVAL_DEVICE && (rc = wait_watching(c, stop))) return rc;
    if ((rc = nla_memcpy_d2h(h_res, c->d_res, sizeof(nla_lbfgs_result) * (size_t) count, c->st))) return rc;
    if ((rc = nla_stream_sync(c->st))) return rc;
    if (c->stats) {
        ++c->stats->lbfgs_launches;
        c->stats->t_lbfgs_ms += (double) nla_event_elapsed_ms(c->ev0, c->ev1);
        for (i = 0; i < count; ++i)
            c->stats->lbfgs_bytes += (uint64_t) c->n * (c->a->bytes_per_col * (uint64_t) h_res[i].cols + c->a->bytes_per_eval * (uint64_t) h_res[i].nevals);
        if (c->alg == NLA_LOCAL_LBFGS) {
            uint64_t longest = 0;
            for (i = 0; i < count; ++i) {
                const uint64_t steps = (uint64_t) c->n * (2ULL * (uint64_t) h_res[i].cols + 4ULL * (uint64_t) h_res[i].nevals);
                if (steps > longest) longest = steps;
            }
            c->stats->lbfgs_longest_chain_steps += longest;
        }
    }
    return 0;
}

/* the context a batch of local searches from host rows runs on (nla_local_run_batch below; nlopt_amd_optimize_batch, batch_driver.c):
 * a stream, the box and the initial step on the device, the context of *spec (its stream, box and step are set here) with the run's
 * options set.  step: LD_MMA's / LN_COBYLA's optional initial step (host, n).  0, or -1 with err filled and everything released. */
int nla_local_batch_open(nla_local_batch *B, const nla_local_spec *spec, const double *lb, const double *ub, const double *step,
                         const nla_stopping *stop, int exact, char *err, size_t errlen)
{
    nla_local_spec s = *spec;
    const int n = s.n, ld = (n + 1) & ~1;
    memset(B, 0, sizeof *B);
    B->n = n; B->ld = ld;
    B->st = nla_stream_create();
    if (!B->st) { snprintf(err, errlen, "stream creation failed"); return -1; }
    B->d_lb = (double *) nla_dev_malloc(sizeof(double) * (size_t) ld);
    B->d_ub = (double *) nla_dev_malloc(sizeof(double) * (size_t) ld);
    if (s.alg != NLA_LOCAL_LBFGS && step) {
        B->d_si = (double *) nla_dev_malloc(sizeof(double) * (size_t) ld);
        if (!B->d_si || nla_memcpy_h2d(B->d_si, step, sizeof(double) * (size_t) n, B->st)) { snprintf(err, errlen, "upload failed"); goto fail; }
    }
    if (!B->d_lb || !B->d_ub) { snprintf(err, errlen, "out of device memory"); goto fail; }
    /* (LN_COBYLA's context reads the box back when it is created: the box is there first, for every algorithm) */
    if (nla_memcpy_h2d(B->d_lb, lb, sizeof(double) * (size_t) n, B->st) || nla_memcpy_h2d(B->d_ub, ub, sizeof(double) * (size_t) n, B->st) ||
        nla_stream_sync(B->st)) { snprintf(err, errlen, "upload failed"); goto fail; }
    s.d_lb = B->d_lb; s.d_ub = B->d_ub; s.d_step = B->d_si; s.stream = B->st;
    B->c = nla_local_ctx_create(&s);
    if (!B->c) { snprintf(err, errlen, "out of device memory"); goto fail; }
    if (nla_local_ctx_set_options(B->c, exact, stop ? stop->xtol_abs : NULL, stop ? stop->x_weights : NULL)) { snprintf(err, errlen, "upload failed"); goto fail; }
    return 0;
fail:
    nla_local_batch_close(B);
    return -1;
}
int nla_local_batch_upload(nla_local_batch *B, int count, const double *h_X, char *err, size_t errlen)
{
    int i;
    for (i = 0; i < count; ++i)
        if (nla_memcpy_h2d(B->c->d_X + (size_t) i * B->ld, h_X + (size_t) i * B->n, sizeof(double) * (size_t) B->n, B->st)) { snprintf(err, errlen, "upload failed"); return -1; }
    return 0;
}
int nla_local_batch_download(nla_local_batch *B, int count, double *h_X, char *err, size_t errlen)
{
    int i;
    for (i = 0; i < count; ++i)
        if (nla_memcpy_d2h(h_X + (size_t) i * B->n, B->c->d_X + (size_t) i * B->ld, sizeof(double) * (size_t) B->n, B->st)) { snprintf(err, errlen, "read-back failed"); return -1; }
    if ((i = nla_stream_sync(B->st))) { snprintf(err, errlen, "read-back failed: %s", nla_dev_error_string(i)); return -1; }
    return 0;
}
void nla_local_batch_close(nla_local_batch *B)
{
    nla_local_ctx_destroy(B->c);
    nla_dev_free(B->d_lb); nla_dev_free(B->d_ub); nla_dev_free(B->d_si);
    if (B->st) nla_stream_destroy(B->st);
    memset(B, 0, sizeof *B);
}

/* spec->cap local searches from the rows of h_X (cap x n, host), results back in h_X / res */
int nla_local_run_batch(const nla_local_spec *spec, const double *lb, const double *ub, const double *step, double *h_X,
                        const nla_lbfgs_params *prm, nla_lbfgs_result *res, const nla_stopping *stop, int exact, int *live_nevals,
                        nlopt_opt trace_to, char *err, size_t errlen)
{
    const int count = spec->cap;
    nla_local_batch B;
    nla_local_ctx *c;
    int rc = -1, i;
    if (nla_local_batch_open(&B, spec, lb, ub, step, stop, exact, err, errlen)) return -1;
    c = B.c;
    if (nla_local_batch_upload(&B, count, h_X, err, errlen)) goto done;
    if (trace_to && trace_to->trace && count == 1 && nla_local_ctx_set_ftrace(c, (int64_t) trace_to->trace_cap)) { snprintf(err, errlen, "out of device memory"); goto done; }
    if ((i = nla_local_ctx_run(c, count, prm, res, stop, live_nevals))) { snprintf(err, errlen, "local-search batch failed: %s", nla_dev_error_string(i)); goto done; }
    if (trace_to && trace_to->trace && count == 1) {
        /* per-evaluation trace (nlopt_amd_set_trace): kind 5 = an objective call of a local search */
        const int64_t calls = spec->alg == NLA_LOCAL_MMA ? res[0].iterm : res[0].nevals;
        const int64_t k = calls < (int64_t) trace_to->trace_cap ? calls : (int64_t) trace_to->trace_cap;
        double *tmp = (double *) malloc(sizeof(double) * (size_t) (k > 0 ? k : 1));
        if (!tmp || (k > 0 && nla_local_ctx_read_ftrace(c, 0, k, tmp))) { free(tmp); snprintf(err, errlen, "trace read-back failed"); goto done; }
        for (i = 0; i < (int) k; ++i) { nlopt_amd_trace_rec *tr = trace_to->trace + i; tr->f = tmp[i]; tr->row = i; tr->kind = 5; tr->accepted = 0; }
        trace_to->trace_len = (size_t) calls;
        free(tmp);
    }
    if (nla_local_batch_download(&B, count, h_X, err, errlen)) goto done;
    rc = 0;
done:
    nla_local_batch_close(&B);
    return rc;
}

/* the stopping values a local search takes from the run's (tolg, LD_LBFGS's own, stays 0 here) */
void nla_local_params_from_stop(nla_lbfgs_params *prm, const nla_stopping *stop)
{
    memset(prm, 0, sizeof *prm);
    prm->minf_max = stop->minf_max; prm->ftol_rel = stop->ftol_rel; prm->ftol_abs = stop->ftol_abs; prm->xtol_rel = stop->xtol_rel;
    prm->maxeval = stop->maxeval;
}

/* one search from x as nlopt_optimize runs it: what nla_lbfgs_minimize (mf, tolg) and nla_mma_minimize (mma, step = opt->dx) share */
nlopt_result nla_local_minimize_one(int alg, nlopt_opt opt, int n, nlopt_func f, void *f_data, const double *lb, const double *ub, double *x,
                                    double *minf, nla_stopping *stop, int mf, double tolg, const nla_mma_params *mma, const double *step)
{
    return nla_local_minimize_one_res(alg, opt, n, f, f_data, lb, ub, x, minf, stop, mf, tolg, mma, step, NULL);
}
nlopt_result nla_local_minimize_one_res(int alg, nlopt_opt opt, int n, nlopt_func f, void *f_data, const double *lb, const double *ub, double *x,
                                        double *minf, nla_stopping *stop, int mf, double tolg, const nla_mma_params *mma, const double *step,
                                        nla_lbfgs_result *res_out)
{
    nla_evaluator ev;
    const nla_local_spec spec = { alg, &ev, n, 1, mf, mma, NULL, NULL, NULL, NULL, NULL, 0, 0, 0, 0, NULL, NULL };   /* (box, step and stream: nla_local_batch_open) */
    nla_lbfgs_params prm;
    nla_lbfgs_result res;
    char err[200];
    if (nla_dev_count() <= 0) { nla_stop_msg(stop, "nlopt_amd: no HIP device visible (this library has no CPU fallback)"); return NLOPT_FAILURE; }
    nla_evaluator_resolve(&ev, opt, f, f_data);
    nla_local_params_from_stop(&prm, stop);
    prm.tolg = tolg;
    if (nla_local_run_batch(&spec, lb, ub, step, x, &prm, &res, stop, nla_exact_mode_for(opt, NULL, &ev),
                            ev.kind == NLA_EVAL_HOST ? stop->nevals_p : NULL, opt, err, sizeof err)) { nla_stop_msg(stop, "device engine: %s", err); return NLOPT_FAILURE; }
    *minf = res.f;
    if (res_out) *res_out = res;
    if (ev.kind != NLA_EVAL_HOST) *stop->nevals_p += res.nevals;       /* host objective: counted call by call */
    return (nlopt_result) res.ret;
}
