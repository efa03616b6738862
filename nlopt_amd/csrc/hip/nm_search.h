/* nm_search.h — the Nelder-Mead search of nldrmd_minimize_ (src/algs/neldermead/nldrmd.c:106-288) by ONE wavefront, once, for both
 * kernels that run it:
 *   hip/nldrmd_kernels.hip  NLOPT_LN_NELDERMEAD: psi = 0 over all n coordinates (SB = false); the header there has the mapping and storage;
 *   hip/sbplx_kernels.hip   NLOPT_LN_SBPLX: sbplx_minimize (src/algs/neldermead/sbplx.c:66-237) around the same steps with psi = 0.25 on
 *                           subspaces of 1 .. 5 coordinates (SB = true); the header there has the outer algorithm's mapping and storage.
 * One copy of each step: the order of the simplex (nm_extreme), close, reflectpt (nm_reflect), CHECK_EVAL (GO_CHECK), the initial simplex
 * with all its bound branches (GO_INIT), reflection / expansion / contraction / shrink (GO_AFTER, GO_SHRINK, GO_TOP), nlopt_stop_x
 * (nm_stop_x).  SB is a template flag: what it adds is discarded from the LN_NELDERMEAD instances at compile time. */
#ifndef NLA_NM_SEARCH_H
#define NLA_NM_SEARCH_H
#include "cobyla_search.h"          /* one wavefront per search: CW_SYNC, the result codes, cw_isinf, cw_tol_reached, cw_default_step */

#define NM_FAILURE (-1)
/* The host's abort flag lies in pinned host memory: a poll is a read across the bus.  Polled behind EVERY evaluation, 4096 searches
 * of the n = 8 Rosenbrock objective (400 evaluations each, 8 us apiece) spent 160 ms in a launch that takes 3.1 ms without any poll —
 * the bus serves about 10 M such reads per second for the whole device; behind every 16th it took 9.6 ms.  Every 64th evaluation of a
 * search: the flag is seen at most 64 evaluations late, in CHECK_EVAL's place as before. */
#define NM_POLL_EVERY 64
/* which evaluation a search is waiting for */
enum { NM_START = 0, NM_INIT = 1, NM_REFLECT = 2, NM_EXPAND = 3, NM_CONTRACT = 4, NM_SHRINK = 5 };

/* distance of two rows of a slice: a whole number of 128-byte lines */
__host__ __device__ static inline int nm_ld(int n) { return (n + 15) & ~15; }
/* doubles of one search's slice: the n + 1 points and the row of initial steps */
__host__ __device__ static inline size_t nm_slice_doubles(int n) { return (size_t) nm_ld(n) * (size_t) (n + 2); }
/* doubles of LDS: the values, the centroid, the trial point, the point under evaluation */
__host__ __device__ static inline size_t nm_vec_doubles(int n) { return 4 * (size_t) n + 1; }

/* the coroutine between two launches: the scalars that are live across an evaluation, behind them the LDS block as it stands */
struct nm_saved {
    double minf, fr, fl, fh, fpred;
    int32_t nevals, stage, idx, ilow, ihigh, pad[3];
};
#define NM_SAVED_DOUBLES ((sizeof(nm_saved) + 7) / 8)
__host__ __device__ static inline size_t nm_save_doubles(int n) { return (NM_SAVED_DOUBLES + nm_vec_doubles(n) + 15) & ~(size_t) 15; }

/* ---- LN_SBPLX (SB = true): sbplx.c:31-32 and the LDS block of one search.  x, xprev, dx, xstep (n doubles each); the sub-simplex — 6 rows
 * of SB_RS doubles, its 6 values, then c, xcur, the trial point, xs, xsstep, lbs, ubs (SB_RS doubles each); the permutation p (n ints) ---- */
#define SB_PSI 0.25
#define SB_OMEGA 0.1
#define SB_NSMIN 2
#define SB_NSMAX 5
#define SB_RS 8
#define SB_SUB_DOUBLES ((SB_NSMAX + 1) * SB_RS + 8 * SB_RS)
__host__ __device__ static inline size_t sb_vec_doubles(int n) { return 4 * (size_t) n + SB_SUB_DOUBLES + ((size_t) n + 1) / 2; }
/* ... and its coroutine between two launches: Nelder-Mead's scalars, the outer algorithm's, behind them the LDS block */
struct sb_saved {
    nm_saved nm;
    double normi, normdx, fdiff, fdiff_max, init_diam;
    int32_t is, ns, nsubs, pad;
};
#define SB_SAVED_DOUBLES ((sizeof(sb_saved) + 7) / 8)
__host__ __device__ static inline size_t sb_save_doubles(int n) { return (SB_SAVED_DOUBLES + sb_vec_doubles(n) + 15) & ~(size_t) 15; }

/* ---- the order of the simplex.  The reference keeps the points in a red-black tree keyed (f, then the point's address): simplex_compare
 * (nldrmd.c:38-43) uses `<`, then `>`, then k1 - k2, which is point index order — a total order, so the tree's shape does not matter:
 * low is the minimum of (f, index), high the maximum, pred(high) the next one down.  Comparisons only, no floating-point sums. ---- */
struct nm_key { double f; int i; };                     /* i < 0: no point */
__device__ static inline int nm_less(nm_key a, nm_key b) { return a.f < b.f || (!(a.f > b.f) && a.i < b.i); }   /* the C comparisons as written: <, >, then index */
template <bool MAX> __device__ static inline nm_key nm_pick(nm_key a, nm_key b)
{
    if (a.i < 0) return b;
    if (b.i < 0) return a;
    return (MAX ? nm_less(a, b) : nm_less(b, a)) ? b : a;
}
/* the greatest (MAX) or least point of fv[0 .. np) other than `skip`: every lane over its points, then the butterfly (the pick is
 * symmetric in its arguments, so both partners of a step hold the same key behind it and all 64 lanes the same one at the end) */
template <bool MAX> __device__ __forceinline__ nm_key nm_extreme(const double *fv, int np, int skip, int lane)
{
    nm_key k = { 0., -1 };
    for (int p = lane; p < np; p += CW_LANES) if (p != skip) { nm_key o = { fv[p], p }; k = nm_pick<MAX>(k, o); }
#define NM_S_(M) { nm_key o; o.f = nla_xor_lane<M>(k.f); o.i = nla_xor_lane<M>(k.i); k = nm_pick<MAX>(k, o); }
    NLA_BUTTERFLY(NM_S_);
#undef NM_S_
    return k;
}

__device__ static inline int nm_close(double a, double b) { return fabs(a - b) <= 1e-13 * (fabs(a) + fabs(b)); }   /* close, nldrmd.c:47-50 */

/* reflectpt (nldrmd.c:63-77): xnew = c + scale (c - xold) pinned to the box; 0 if xnew coincides with c or with xold.  xnew may be xold
 * (the in-place expansion, nldrmd.c:238): every coordinate is read before it is written, by the lane that owns it. */
__device__ __forceinline__ int nm_reflect(int n, double *xnew, const double *c, double scale, const double *xold, const double *lb,
                                          const double *ub, lb_shared &S, int lane)
{
    int neqc = 0, neqold = 0;
    for (int j = lane; j < n; j += CW_LANES) {
        const double cj = c[j], oj = xold[j];
        double newx = cj + scale * (cj - oj);                /* one multiply, a subtraction and an addition: never an FMA (contraction is off) */
        if (newx < lb[j]) newx = lb[j];                      /* the clamps in the reference's order: lb first, then ub */
        if (newx > ub[j]) newx = ub[j];
        neqc |= !nm_close(newx, cj);
        neqold |= !nm_close(newx, oj);
        xnew[j] = newx;
    }
    /* equalc / equalold: wave-wide ANDs over the coordinates */
    const int anyc = lb_block_isum(neqc, S), anyold = lb_block_isum(neqold, S);
    CW_SYNC();
    return !(anyc == 0 || anyold == 0);
}

/* nlopt_stop_x(stop, x, oldx) (stop.c:98-108) over n coordinates in LDS: the two weighted L1 norms (stop.c:37-79) in ascending coordinate
 * order, whatever `exact` is, with `<`; then the xtol_abs test with `>=`.  Every lane calls it and gets the same answer. */
__device__ __forceinline__ int nm_stop_x(int n, const double *x, const double *oldx, const nla_nldrmd_params &P, lb_shared &S, lb_exact_buf &XB, int lane)
{
    double dnorm = 0., xnorm = 0.;
    const double *w = P.x_weights;
    lb_seq_sum2<false>(0, n, &dnorm, &xnorm, [&](int i, double *pa, double *pb) {
        *pa = w ? w[i] * fabs(x[i] - oldx[i]) : fabs(x[i] - oldx[i]);
        *pb = w ? w[i] * fabs(x[i]) : fabs(x[i]);
    }, XB);
    int stop = dnorm < P.xtol_rel * xnorm;                /* `<` on the norms */
    if (!stop && P.xtol_abs) {
        int over = 0;
        for (int j = lane; j < n; j += CW_LANES) if (fabs(x[j] - oldx[j]) >= P.xtol_abs[j]) over = 1;      /* `>=` on the xtol_abs test */
        stop = lb_block_isum(over, S) == 0;
    }
    return stop;
}

/* ONE search by one wavefront.  EXT = false: the objective OBJ is compiled in, P.abort is polled behind every NM_POLL_EVERY-th evaluation, P.done counts
 * the finished searches.  EXT = true: the coroutine (E as in include/nlopt_amd.h); OBJ, oscratch and XB's role for the objective unused.
 * SB = false: vec is the LDS block (nm_vec_doubles(N)), pts_g this search's slice.  SB = true: vec is the LDS block (sb_vec_doubles(N)),
 * pts_g unused; n, the dimension the Nelder-Mead steps work on, is the current subspace's. */
template <int OBJ, bool EXT, bool SB = false>
__device__ __forceinline__ void nm_search(int N, int ld, int count, const double *__restrict__ lb_g, const double *__restrict__ ub_g,
                                          const double *__restrict__ dx_given, double *__restrict__ X, nla_nldrmd_params P,
                                          nla_lbfgs_result *__restrict__ out, double *vec, double *pts_g, lb_shared &S, double *oscratch,
                                          lb_exact_buf &XB, const nla_local_ext &E = nla_local_ext())
{
    const int inst = blockIdx.x, lane = threadIdx.x;
    if (inst >= count) return;
    /* a launch that resumes concerns the searches that wait for their value (state 1): a finished one (2) stays as it is.  (Every lane
     * reads the same word, and a barrier stands between this read and the store that ends the launch.) */
    if (EXT && E.resume && E.req[inst].state != 1) return;
    const bool resumed = EXT && E.resume;
    const int rs = SB ? SB_RS : nm_ld(N);
    int n = N;                                                    /* (SB: the subspace's) */
    nm_saved *sv = EXT ? (nm_saved *) ((double *) E.save + (size_t) inst * (SB ? sb_save_doubles(N) : nm_save_doubles(N))) : nullptr;
    sb_saved *sbv = (sb_saved *) sv;
    double *svec = EXT ? (double *) sv + (SB ? SB_SAVED_DOUBLES : NM_SAVED_DOUBLES) : nullptr;
    double *xrow = X + (size_t) inst * ld;                        /* the reference's x: the start, then the best point seen (SB: at the end) */
    /* SB: the full-length vectors and the subspace's block behind them */
    double *xfull = vec, *xprev = vec + N, *dxv = xprev + N, *xstep = dxv + N, *sub = xstep + N;
    double *lbs = sub + (SB_NSMAX + 1) * SB_RS + 6 * SB_RS, *ubs = lbs + SB_RS;
    int *perm = (int *) (sub + SB_SUB_DOUBLES);
    double *pts = SB ? sub : pts_g;
    double *fv = SB ? sub + (SB_NSMAX + 1) * SB_RS : vec, *c = SB ? fv + SB_RS : fv + (N + 1), *xcur = SB ? c + SB_RS : c + N, *xev = SB ? xcur + SB_RS : xcur + N;
    double *x0 = SB ? xev + SB_RS : xrow;                         /* the x of nldrmd_minimize_ (SB: xs) */
    double *steps = SB ? x0 + SB_RS : pts + (size_t) rs * (N + 1);
    const double *lb = SB ? lbs : lb_g, *ub = SB ? ubs : ub_g;
    const size_t total = SB ? sb_vec_doubles(N) : nm_vec_doubles(N);
    const double ALPHA = 1, BETA = 0.5, GAMMA = 2, DELTA = 0.5;   /* nldrmd.c:35 */
    double ninv = 1.0 / n;
    enum { GO_EVAL, GO_CHECK, GO_AFTER, GO_INIT, GO_SHRINK, GO_TOP, GO_PASS, GO_SUB, GO_SUBEND, GO_PASSEND, GO_DONE };
    const int GO_END = SB ? GO_SUBEND : GO_DONE;                  /* where nldrmd_minimize_ returns to */
    double minf = __builtin_huge_val(), f = 0., fr = 0., fl = 0., fh = 0., fpred = 0.;
    double normi = 0., normdx = 0., fdiff = 0., fdiff_max = 0., init_diam = 0.;
    int nevals = 0, stage = NM_START, idx = 0, ilow = 0, ihigh = 0, rc = CW_SUCCESS, faildim = 0, go = GO_EVAL, forced = 0, timed = 0;
    int is = 0, nsubs = 0;

    if (resumed) {
        for (size_t e = lane; e < total; e += CW_LANES) vec[e] = svec[e];
        minf = sv->minf; fr = sv->fr; fl = sv->fl; fh = sv->fh; fpred = sv->fpred;
        nevals = sv->nevals; stage = sv->stage; idx = sv->idx; ilow = sv->ilow; ihigh = sv->ihigh;
        if (SB) {
            normi = sbv->normi; normdx = sbv->normdx; fdiff = sbv->fdiff; fdiff_max = sbv->fdiff_max; init_diam = sbv->init_diam;
            is = sbv->is; n = sbv->ns; nsubs = sbv->nsubs; ninv = 1.0 / n;
        }
        f = E.EF[inst];                                           /* as delivered: the caller has applied the sign */
        go = GO_CHECK;
    } else if (SB) {
        /* the initial step as below; dx = 0: the first pass's permutation is the identity */
        for (int j = lane; j < N; j += CW_LANES) {
            const double xj = xrow[j];
            xstep[j] = dx_given ? dx_given[j] : cw_default_step(lb_g[j], ub_g[j], xj);
            xfull[j] = xj;
            dxv[j] = 0.;
        }
    } else {
        /* the initial step: the caller's, or nlopt_set_default_initial_step at the START point (optimize.c:891-903); point 0 = the start */
        for (int j = lane; j < n; j += CW_LANES) {
            const double xj = x0[j];
            steps[j] = dx_given ? dx_given[j] : cw_default_step(lb[j], ub[j], xj);
            pts[j] = xj;
            xev[j] = xj;
        }
    }
    if (EXT) { forced = E.forced; timed = E.timeout; }            /* the caller's verdicts at this launch */
    CW_SYNC();

    while (go != GO_DONE) switch (go) {
    case GO_EVAL: {                                               /* f at xev */
        /* SB: subspace_func (sbplx.c:54-64) scatters the trial point into the full x, and the full x is what is evaluated */
        if (SB) {
            if (stage != NM_START) for (int j = lane; j < n; j += CW_LANES) xfull[perm[is + j]] = xev[j];
            CW_SYNC();
        }
        const double *xe = SB ? xfull : xev;
        if (EXT) {                                                /* the coroutine leaves: the point, the LDS block, the scalars, the request */
            for (int j = lane; j < N; j += CW_LANES) E.EX[(size_t) inst * ld + j] = xe[j];
            for (size_t e = lane; e < total; e += CW_LANES) svec[e] = vec[e];
            if (lane == 0) {
                sv->minf = minf; sv->fr = fr; sv->fl = fl; sv->fh = fh; sv->fpred = fpred;
                sv->nevals = nevals; sv->stage = stage; sv->idx = idx; sv->ilow = ilow; sv->ihigh = ihigh;
                if (SB) {
                    sbv->normi = normi; sbv->normdx = normdx; sbv->fdiff = fdiff; sbv->fdiff_max = fdiff_max; sbv->init_diam = init_diam;
                    sbv->is = is; sbv->ns = n; sbv->nsubs = nsubs;
                }
                E.req[inst].state = 1; E.req[inst].want_grad = 0;
            }
            return;
        }
        /* summed as the other local kernels sum it: the wave tree with the bits of their 256-thread reduction, or the reference's
         * sequential order (exact) */
        if (P.exact) { nla_obj_part t; f = lb_obj_exact<OBJ>(N, xe, &t, XB); }
        else f = nla_block_objective_as<OBJ, 1, 4>(N, [&](int q) { return xe[q]; }, oscratch);
        f *= P.sign;
    }
    /* fall through */
    case GO_CHECK: {                                              /* CHECK_EVAL (nldrmd.c:79-87); the first evaluation: nldrmd.c:300-305, sbplx.c:79-84 */
        if (P.ftrace && lane == 0 && nevals < P.ftrace_cap) P.ftrace[(size_t) inst * P.ftrace_cap + nevals] = f;
        ++nevals;                                                 /* 1: count */
        if (!EXT && P.abort && (nevals & (NM_POLL_EVERY - 1)) == 0) { const int ab = lb_poll_abort(P.abort); forced = ab == -999; timed = ab == 100; }
        if (stage == NM_START) minf = f;
        if (forced) { rc = CW_FORCED_STOP; go = stage == NM_START ? GO_DONE : GO_END; break; } /* 2: forced stop */
        if (stage == NM_START) { if (minf < P.minf_max) rc = CW_MINF_MAX_REACHED; }
        else if (f <= minf) {                                     /* 3: the best point with <= (a later equal value replaces x), the stop value with < */
            minf = f;
            CW_SYNC();
            for (int j = lane; j < n; j += CW_LANES) x0[j] = xev[j];
            CW_SYNC();
            if (minf < P.minf_max) rc = CW_MINF_MAX_REACHED;
        }
        if (rc == CW_SUCCESS) {
            if (P.maxeval > 0 && nevals >= P.maxeval) rc = CW_MAXEVAL_REACHED;      /* 4: maxeval */
            else if (timed) rc = CW_MAXTIME_REACHED;                                /* 5: time */
        }
        go = rc == CW_SUCCESS ? GO_AFTER : stage == NM_START ? GO_DONE : GO_END;
        break;
    }
    case GO_AFTER: {                                              /* behind a counted evaluation: what the reference does with the value */
        CW_SYNC();
        switch (stage) {
        case NM_START:
            if (SB) { go = GO_PASS; break; }
            if (lane == 0) fv[0] = minf;
            idx = 0; go = GO_INIT;
            break;
        case NM_INIT:
            if (lane == 0) fv[idx + 1] = f;
            ++idx; go = idx < n ? GO_INIT : GO_TOP;
            break;
        case NM_REFLECT: {
            double *xh = pts + (size_t) rs * ihigh;
            fr = f;
            if (fr < fl) {                                        /* new best point: expand, in place (nldrmd.c:237-242) */
                if (!nm_reflect(n, xh, c, GAMMA, xh, lb, ub, S, lane)) { rc = CW_XTOL_REACHED; go = GO_END; break; }
                for (int j = lane; j < n; j += CW_LANES) xev[j] = xh[j];
                stage = NM_EXPAND; go = GO_EVAL;
            } else if (fr < fpred) {                              /* accept the new point (nldrmd.c:248-251) */
                for (int j = lane; j < n; j += CW_LANES) xh[j] = xcur[j];
                if (lane == 0) fv[ihigh] = fr;
                go = GO_TOP;
            } else {                                              /* new worst point: contract (nldrmd.c:252-258) */
                if (!nm_reflect(n, xcur, c, fh <= fr ? -BETA : BETA, xh, lb, ub, S, lane)) { rc = CW_XTOL_REACHED; go = GO_END; break; }
                for (int j = lane; j < n; j += CW_LANES) xev[j] = xcur[j];
                stage = NM_CONTRACT; go = GO_EVAL;
            }
            break;
        }
        case NM_EXPAND: {
            double *xh = pts + (size_t) rs * ihigh;
            double fe = f;
            if (fe >= fr) {                                       /* expanding did not improve (nldrmd.c:243-246) */
                fe = fr;
                for (int j = lane; j < n; j += CW_LANES) xh[j] = xcur[j];
            }
            if (lane == 0) fv[ihigh] = fe;
            go = GO_TOP;
            break;
        }
        case NM_CONTRACT:
            if (f < fr && f < fh) {                               /* successful contraction (nldrmd.c:259-262) */
                double *xh = pts + (size_t) rs * ihigh;
                for (int j = lane; j < n; j += CW_LANES) xh[j] = xcur[j];
                if (lane == 0) fv[ihigh] = f;
                go = GO_TOP;
            } else { idx = 0; go = GO_SHRINK; }                   /* failed: shrink the simplex */
            break;
        default:                                                  /* NM_SHRINK */
            if (lane == 0) fv[idx] = f;
            ++idx; go = GO_SHRINK;
            break;
        }
        CW_SYNC();
        break;
    }
    case GO_INIT: {                                               /* point idx + 1 of the initial simplex (nldrmd.c:136-163), ALL branches; x = x0, the
                                                                   * best point so far, as the reference's CHECK_EVAL has left it */
        double *pt = pts + (size_t) rs * (idx + 1);
        const double xi = x0[idx], st = steps[idx], lo = lb[idx], hi = ub[idx];
        double v = xi + st;
        if (v > hi) {
            if (hi - xi > fabs(st) * 0.1) v = hi;
            else v = xi - fabs(st);                               /* ub is too close: the other direction */
        }
        if (v < lo) {
            if (xi - lo > fabs(st) * 0.1) v = lo;
            else {                                                /* lb is too close: the other direction, or towards the further bound */
                v = xi + fabs(st);
                if (v > hi) v = 0.5 * ((hi - xi > xi - lo ? hi : lo) + xi);
            }
        }
        /* the step is too small: NLOPT_FAILURE, the dimension in the result record, no further evaluation, X as it is */
        if (nm_close(v, xi)) { rc = NM_FAILURE; faildim = idx; go = GO_END; break; }
        for (int j = lane; j < n; j += CW_LANES) { const double pj = j == idx ? v : x0[j]; pt[j] = pj; xev[j] = pj; }
        CW_SYNC();
        stage = NM_INIT; go = GO_EVAL;
        break;
    }
    case GO_SHRINK: {                                             /* nldrmd.c:263-278: the points in index order, skipping low, one evaluation each */
        if (idx == ilow) ++idx;
        if (idx > n) { go = GO_TOP; break; }                      /* "goto restart": the order is taken anew */
        double *pt = pts + (size_t) rs * idx;
        if (!nm_reflect(n, pt, pts + (size_t) rs * ilow, -DELTA, pt, lb, ub, S, lane)) { rc = CW_XTOL_REACHED; go = GO_END; break; }
        for (int j = lane; j < n; j += CW_LANES) xev[j] = pt[j];
        CW_SYNC();
        stage = NM_SHRINK; go = GO_EVAL;
        break;
    }
    case GO_TOP: {                                                /* one iteration up to its reflection (nldrmd.c:173-234) */
        const nm_key klow = nm_extreme<false>(fv, n + 1, -1, lane), khigh = nm_extreme<true>(fv, n + 1, -1, lane);
        const nm_key kpred = nm_extreme<true>(fv, n + 1, khigh.i, lane);       /* (n >= 1: there is one) */
        ilow = klow.i; ihigh = khigh.i; fl = klow.f; fh = khigh.f; fpred = kpred.f;
        if (SB) {
            /* psi > 0: *fdiff at every iteration top, also behind a shrink; the diameter |xl - xh| of the first simplex (while it is 0),
             * summed in ascending coordinate by every lane; no ftol test (nldrmd.c:180-188) */
            fdiff = fh - fl;
            if (init_diam == 0) for (int i = 0; i < n; ++i) init_diam += fabs(pts[rs * ilow + i] - pts[rs * ihigh + i]);
        }
        /* nlopt_stop_ftol(stop, fl, fh): relstop of stop.c:81-86 with the isinf(vold) guard */
        else if (cw_tol_reached(fh, fl, P.ftol_rel, P.ftol_abs)) { rc = CW_FTOL_REACHED; go = GO_END; break; }
        /* the centroid (nldrmd.c:195-202): lane j adds coordinate j over the points in index order, skipping high, then MULTIPLIES by
         * ninv = 1.0 / n; recomputed every iteration — an incrementally updated centroid changes the bits */
        for (int j = lane; j < n; j += CW_LANES) {
            double cj = 0.;
            for (int i = 0; i <= n; ++i) if (i != ihigh) cj += pts[(size_t) rs * i + j];
            c[j] = cj * ninv;
        }
        if (SB) {
            /* diam < psi * init_diam REPLACES nlopt_stop_x (nldrmd.c:217-224); xcur, the greatest radius, is not needed then */
            double diam = 0.;
            for (int i = 0; i < n; ++i) diam += fabs(pts[rs * ilow + i] - pts[rs * ihigh + i]);
            if (diam < SB_PSI * init_diam) { rc = CW_XTOL_REACHED; go = GO_END; break; }
        }
        /* nlopt_stop_x(stop, c, xcur) with xcur = the greatest radius from the centroid (nldrmd.c:204-228).  With xtol_rel <= 0 and no
         * xtol_abs the test cannot hold (stop.c:101-103: a norm is never < 0 or < NaN), and reflectpt overwrites xcur: skipped then */
        else if (P.xtol_rel > 0 || P.xtol_abs) {
            for (int j = lane; j < n; j += CW_LANES) {
                const double cj = c[j];
                double r = 0.;
                for (int i = 0; i <= n; ++i) { const double d = fabs(pts[(size_t) rs * i + j] - cj); if (d > r) r = d; }
                xcur[j] = r + cj;
            }
            if (nm_stop_x(n, c, xcur, P, S, XB, lane)) { rc = CW_XTOL_REACHED; go = GO_END; break; }
        }
        CW_SYNC();
        if (!nm_reflect(n, xcur, c, ALPHA, pts + (size_t) rs * ihigh, lb, ub, S, lane)) { rc = CW_XTOL_REACHED; go = GO_END; break; }
        for (int j = lane; j < n; j += CW_LANES) xev[j] = xcur[j];
        CW_SYNC();
        stage = NM_REFLECT; go = GO_EVAL;
        break;
    }
    /* ---- LN_SBPLX only (sbplx.c:105-231); no LN_NELDERMEAD instance reaches or keeps what follows ---- */
    case GO_PASS: {                                               /* the top of a pass: xprev, the permutation, normdx (sbplx.c:106-120) */
        if (!SB) { go = GO_DONE; break; }
        for (int j = lane; j < N; j += CW_LANES) { xprev[j] = xfull[j]; perm[j] = j; }
        CW_SYNC();
        /* p: the indices by decreasing |dx|, ties in index order — nlopt_qsort_r is glibc's qsort_r in the reference's build, a merge sort
         * at these sizes, so stable.  The rank of i: #{j : |dx_j| > |dx_i|} + #{j < i : |dx_j| == |dx_i|}; comparisons only.  (p starts as
         * the identity so that a NaN in dx, whose ranks collide, still leaves indices below N in every place) */
        for (int i = lane; i < N; i += CW_LANES) {
            const double a = fabs(dxv[i]);
            int r = 0;
            for (int j = 0; j < N; ++j) { const double b = fabs(dxv[j]); r += (b > a || (b == a && j < i)) ? 1 : 0; }
            perm[r] = i;
        }
        CW_SYNC();
        normdx = 0.;
        for (int i = 0; i < N; ++i) normdx += fabs(dxv[i]);       /* index order, by every lane */
        normi = 0.; nsubs = 0; fdiff_max = 0.; is = 0;
        go = GO_SUB;
        break;
    }
    case GO_SUB: {                                                /* the subspace that starts at is: its size (sbplx.c:121-144, or the last one, :166),
                                                                   * its point, step and box (:147-152), the entry of nldrmd_minimize_ (nldrmd.c:130-135) */
        if (!SB) { go = GO_DONE; break; }
        if (is + SB_NSMIN < N) {
            double ns_goodness = -__builtin_huge_val(), norm = normi;
            const int nk = is + SB_NSMAX > N ? N : is + SB_NSMAX;
            int k;
            for (k = is; k < is + SB_NSMIN - 1; ++k) norm += fabs(dxv[perm[k]]);
            n = SB_NSMIN;
            for (k = is + SB_NSMIN - 1; k < nk; ++k) {
                double goodness;
                norm += fabs(dxv[perm[k]]);
                if (N - (k + 1) < SB_NSMIN) continue;             /* remaining subspaces must be big enough to partition */
                if (k + 1 < N) goodness = norm / (k + 1) - (normdx - norm) / (N - (k + 1));
                else goodness = normdx / N;
                if (goodness > ns_goodness) { ns_goodness = goodness; n = (k + 1) - is; }
            }
            for (k = is; k < is + n; ++k) normi += fabs(dxv[perm[k]]);
        } else n = N - is;
        for (int k = lane; k < n; k += CW_LANES) {
            const int q = perm[is + k];
            const double xq = xfull[q];
            x0[k] = xq; pts[k] = xq; steps[k] = xstep[q]; lbs[k] = lb_g[q]; ubs[k] = ub_g[q];
        }
        if (lane == 0) fv[0] = minf;                              /* pts[0] takes *minf with no evaluation */
        ++nsubs;
        ninv = 1.0 / n;
        fdiff = __builtin_huge_val(); init_diam = 0.;
        CW_SYNC();
        if (minf < P.minf_max) { rc = CW_MINF_MAX_REACHED; go = GO_SUBEND; break; }
        idx = 0; go = GO_INIT;
        break;
    }
    case GO_SUBEND: {                                             /* behind nldrmd_minimize_ (sbplx.c:157-163, :178-184) */
        if (!SB) { go = GO_DONE; break; }
        CW_SYNC();
        for (int k = lane; k < n; k += CW_LANES) xfull[perm[is + k]] = x0[k];      /* the best back into x before any `goto done` */
        CW_SYNC();
        if (fdiff > fdiff_max) fdiff_max = fdiff;
        /* a too-small step ends the WHOLE search with XTOL_REACHED; 1 + the subspace's dimension in the result record */
        if (rc == NM_FAILURE) { rc = CW_XTOL_REACHED; faildim = idx + 1; go = GO_DONE; break; }
        if (rc != CW_XTOL_REACHED) { go = GO_DONE; break; }
        rc = CW_SUCCESS;
        if (is + SB_NSMIN < N) { is += n; go = GO_SUB; }          /* (this one came out of the loop: the loop's `i += ns`) */
        else go = GO_PASSEND;
        break;
    }
    case GO_PASSEND: {                                            /* the end of a pass (sbplx.c:186-230) */
        if (!SB) { go = GO_DONE; break; }
        if (cw_tol_reached(minf + fdiff_max, minf, P.ftol_rel, P.ftol_abs)) { rc = CW_FTOL_REACHED; go = GO_DONE; break; }
        /* nlopt_stop_x(x, xprev) and then |xstep| psi on every coordinate (with xtol_rel <= 0 and no xtol_abs the first cannot hold, as above) */
        if ((P.xtol_rel > 0 || P.xtol_abs) && nm_stop_x(N, xfull, xprev, P, S, XB, lane)) {
            int big = 0;
            for (int j = lane; j < N; j += CW_LANES) {
                const double s = fabs(xstep[j]) * SB_PSI;
                if (s > (P.xtol_abs ? P.xtol_abs[j] : 0) && s > P.xtol_rel * fabs(xfull[j])) big = 1;
            }
            if (lb_block_isum(big, S) == 0) { rc = CW_XTOL_REACHED; go = GO_DONE; break; }
        }
        CW_SYNC();
        for (int j = lane; j < N; j += CW_LANES) dxv[j] = xfull[j] - xprev[j];
        CW_SYNC();
        double scale;
        if (nsubs == 1) scale = SB_PSI;
        else {
            double stepnorm = 0., dxnorm = 0.;
            for (int i = 0; i < N; ++i) { stepnorm += fabs(xstep[i]); dxnorm += fabs(dxv[i]); }      /* index order, by every lane */
            scale = dxnorm / stepnorm;
            if (scale < SB_OMEGA) scale = SB_OMEGA;
            if (scale > 1 / SB_OMEGA) scale = 1 / SB_OMEGA;
        }
        CW_SYNC();
        for (int j = lane; j < N; j += CW_LANES) {
            const double s = xstep[j] * scale;
            xstep[j] = dxv[j] == 0 ? -s : copysign(s, dxv[j]);
        }
        CW_SYNC();
        go = GO_PASS;
        break;
    }
    }
    /* X row `inst` holds the best point seen, minf its value */
    if (SB) {
        CW_SYNC();
        for (int j = lane; j < N; j += CW_LANES) xrow[j] = xfull[j];
    }
    if (lane == 0) {
        out[inst].f = minf; out[inst].ret = rc; out[inst].nevals = nevals; out[inst].iterm = nevals; out[inst].cols = faildim;
        if (EXT) { E.req[inst].state = 2; E.req[inst].want_grad = 0; }
        else if (P.done) __hip_atomic_fetch_add(P.done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
#endif
