/* nldrmd_kernels.hip — batched NLOPT_LN_NELDERMEAD: replaces nldrmd_minimize with psi = 0 (src/algs/neldermead/nldrmd.c:290-314 over
 * nldrmd_minimize_, :106-288) as nlopt_optimize reaches it (optimize.c:886-905) for `count` independent starts at once, one WAVEFRONT per
 * start (one wavefront per workgroup, as the COBYLA kernels: a launch spreads thousands of searches over the compute units).  The search
 * body exists once (nm_search) and is instantiated
 *   nldrmd_batch_kernel<OBJ>   for a compiled-in device objective: the whole search is one launch;
 *   nldrmd_batch_ext_kernel    as a COROUTINE by the "External evaluation" contract of include/nlopt_amd.h: a launch runs every search
 *                              from where it stands to its next evaluation — the point goes to row `inst` of EX, req[inst] = {1, 0} — or
 *                              to its end (req[inst].state = 2) and ENDS; the caller evaluates, writes EF and launches again with
 *                              resume = 1.  want_grad is always 0, EF[inst] is taken as delivered, ext->forced / ext->timeout stand where
 *                              the reference's CHECK_EVAL asks nlopt_stop_forced / nlopt_stop_time, a finished search stays finished
 *                              through later launches, and a launch waits for nothing.
 *
 * Mapping.  Every coordinate loop of Nelder-Mead is independent per coordinate: lane l owns coordinates l, l + 64, ... of every point, in
 * every loop, so a lane only ever reads coordinates it wrote itself and each result is the reference's bit for bit with no cross-lane
 * sum.  What does cross lanes: the order of the simplex (comparisons only), the wave-wide ANDs of reflectpt, the two norms of the x-stop
 * test (summed in ascending coordinate order by every lane from LDS) and the objective.
 *
 * Storage.  The simplex — n + 1 rows of n coordinates — and the initial steps (one more row) live in the search's slice of `work`: rows
 * nm_ld(n) doubles apart, a whole number of 128-byte lines, the slice on a 128-byte boundary, so lane j reading coordinate j of a row is
 * one coalesced access.  The n + 1 function values, the centroid, the trial point and the point under evaluation live in LDS (4n + 1
 * doubles).  Between two launches of the coroutine those vectors and the live scalars (nm_saved) lie in the search's record of
 * ext->save; the slice and row `inst` of X (the best point seen, as the reference keeps it in x) are in device memory anyway.  A slice and
 * a record belong to ONE wavefront; what one launch stored the next reads across the kernel boundary: no fence, no atomic, no flag.
 *
 * Bound by: per iteration one or two passes over the (n + 1) n doubles of the simplex (a few KB at n <= 16: L2 / L1 hits), their load
 * latency in the n + 1 dependent additions of the centroid, and, for the coroutine, one kernel launch plus the record out and in per
 * evaluation — latency and launches, not bandwidth.  No scratch memory, no private arrays: the per-lane state is a handful of doubles.
 *
 * Out of scope: NLOPT_LN_SBPLX (it calls nldrmd_minimize_ with psi > 0), LN_NELDERMEAD as MLSL's local optimiser (mlsl_check_args keeps
 * its message), multi-rank batches, n > NLA_NLDRMD_MAX_N = 256.  A NaN objective value is outside the parity contract: the search still
 * ends at maxeval and disturbs no other search. */
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

/* ONE search by one wavefront.  EXT = false: the objective OBJ is compiled in, P.abort is polled behind every NM_POLL_EVERY-th evaluation, P.done counts
 * the finished searches.  EXT = true: the coroutine (E as in include/nlopt_amd.h); OBJ, oscratch and XB's role for the objective unused.
 * vec: the LDS block (nm_vec_doubles(n)); pts: this search's slice. */
template <int OBJ, bool EXT>
__device__ __forceinline__ void nm_search(int n, int ld, int count, const double *__restrict__ lb, const double *__restrict__ ub,
                                          const double *__restrict__ dx_given, double *__restrict__ X, nla_nldrmd_params P,
                                          nla_lbfgs_result *__restrict__ out, double *vec, double *pts, lb_shared &S, double *oscratch,
                                          lb_exact_buf &XB, const nla_local_ext &E = nla_local_ext())
{
    const int inst = blockIdx.x, lane = threadIdx.x;
    if (inst >= count) return;
    /* a launch that resumes concerns the searches that wait for their value (state 1): a finished one (2) stays as it is.  (Every lane
     * reads the same word, and a barrier stands between this read and the store that ends the launch.) */
    if (EXT && E.resume && E.req[inst].state != 1) return;
    const bool resumed = EXT && E.resume;
    const int rs = nm_ld(n);
    nm_saved *sv = EXT ? (nm_saved *) ((double *) E.save + (size_t) inst * nm_save_doubles(n)) : nullptr;
    double *svec = EXT ? (double *) sv + NM_SAVED_DOUBLES : nullptr;
    double *x0 = X + (size_t) inst * ld;                          /* the reference's x: the start, then the best point seen */
    double *fv = vec, *c = fv + (n + 1), *xcur = c + n, *xev = xcur + n;
    double *steps = pts + (size_t) rs * (n + 1);
    const size_t total = nm_vec_doubles(n);
    const double ALPHA = 1, BETA = 0.5, GAMMA = 2, DELTA = 0.5;   /* nldrmd.c:35 */
    const double ninv = 1.0 / n;
    enum { GO_EVAL, GO_CHECK, GO_AFTER, GO_INIT, GO_SHRINK, GO_TOP, GO_DONE };
    double minf = __builtin_huge_val(), f = 0., fr = 0., fl = 0., fh = 0., fpred = 0.;
    int nevals = 0, stage = NM_START, idx = 0, ilow = 0, ihigh = 0, rc = CW_SUCCESS, faildim = 0, go = GO_EVAL, forced = 0, timed = 0;

    if (resumed) {
        for (size_t e = lane; e < total; e += CW_LANES) vec[e] = svec[e];
        minf = sv->minf; fr = sv->fr; fl = sv->fl; fh = sv->fh; fpred = sv->fpred;
        nevals = sv->nevals; stage = sv->stage; idx = sv->idx; ilow = sv->ilow; ihigh = sv->ihigh;
        f = E.EF[inst];                                           /* as delivered: the caller has applied the sign */
        go = GO_CHECK;
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
        if (EXT) {                                                /* the coroutine leaves: the point, the LDS block, the scalars, the request */
            for (int j = lane; j < n; j += CW_LANES) E.EX[(size_t) inst * ld + j] = xev[j];
            for (size_t e = lane; e < total; e += CW_LANES) svec[e] = vec[e];
            if (lane == 0) {
                sv->minf = minf; sv->fr = fr; sv->fl = fl; sv->fh = fh; sv->fpred = fpred;
                sv->nevals = nevals; sv->stage = stage; sv->idx = idx; sv->ilow = ilow; sv->ihigh = ihigh;
                E.req[inst].state = 1; E.req[inst].want_grad = 0;
            }
            return;
        }
        /* summed as the other local kernels sum it: the wave tree with the bits of their 256-thread reduction, or the reference's
         * sequential order (exact) */
        if (P.exact) { nla_obj_part t; f = lb_obj_exact<OBJ>(n, xev, &t, XB); }
        else f = nla_block_objective_as<OBJ, 1, 4>(n, [&](int q) { return xev[q]; }, oscratch);
        f *= P.sign;
    }
    /* fall through */
    case GO_CHECK: {                                              /* CHECK_EVAL (nldrmd.c:79-87); the first evaluation: nldrmd.c:300-305 */
        if (P.ftrace && lane == 0 && nevals < P.ftrace_cap) P.ftrace[(size_t) inst * P.ftrace_cap + nevals] = f;
        ++nevals;                                                 /* 1: count */
        if (!EXT && P.abort && (nevals & (NM_POLL_EVERY - 1)) == 0) { const int ab = lb_poll_abort(P.abort); forced = ab == -999; timed = ab == 100; }
        if (stage == NM_START) minf = f;
        if (forced) { rc = CW_FORCED_STOP; go = GO_DONE; break; } /* 2: forced stop */
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
        go = rc == CW_SUCCESS ? GO_AFTER : GO_DONE;
        break;
    }
    case GO_AFTER: {                                              /* behind a counted evaluation: what the reference does with the value */
        CW_SYNC();
        switch (stage) {
        case NM_START:
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
                if (!nm_reflect(n, xh, c, GAMMA, xh, lb, ub, S, lane)) { rc = CW_XTOL_REACHED; go = GO_DONE; break; }
                for (int j = lane; j < n; j += CW_LANES) xev[j] = xh[j];
                stage = NM_EXPAND; go = GO_EVAL;
            } else if (fr < fpred) {                              /* accept the new point (nldrmd.c:248-251) */
                for (int j = lane; j < n; j += CW_LANES) xh[j] = xcur[j];
                if (lane == 0) fv[ihigh] = fr;
                go = GO_TOP;
            } else {                                              /* new worst point: contract (nldrmd.c:252-258) */
                if (!nm_reflect(n, xcur, c, fh <= fr ? -BETA : BETA, xh, lb, ub, S, lane)) { rc = CW_XTOL_REACHED; go = GO_DONE; break; }
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
        if (nm_close(v, xi)) { rc = NM_FAILURE; faildim = idx; go = GO_DONE; break; }
        for (int j = lane; j < n; j += CW_LANES) { const double pj = j == idx ? v : x0[j]; pt[j] = pj; xev[j] = pj; }
        CW_SYNC();
        stage = NM_INIT; go = GO_EVAL;
        break;
    }
    case GO_SHRINK: {                                             /* nldrmd.c:263-278: the points in index order, skipping low, one evaluation each */
        if (idx == ilow) ++idx;
        if (idx > n) { go = GO_TOP; break; }                      /* "goto restart": the order is taken anew */
        double *pt = pts + (size_t) rs * idx;
        if (!nm_reflect(n, pt, pts + (size_t) rs * ilow, -DELTA, pt, lb, ub, S, lane)) { rc = CW_XTOL_REACHED; go = GO_DONE; break; }
        for (int j = lane; j < n; j += CW_LANES) xev[j] = pt[j];
        CW_SYNC();
        stage = NM_SHRINK; go = GO_EVAL;
        break;
    }
    case GO_TOP: {                                                /* one iteration up to its reflection (nldrmd.c:173-234) */
        const nm_key klow = nm_extreme<false>(fv, n + 1, -1, lane), khigh = nm_extreme<true>(fv, n + 1, -1, lane);
        const nm_key kpred = nm_extreme<true>(fv, n + 1, khigh.i, lane);       /* (n >= 1: there is one) */
        ilow = klow.i; ihigh = khigh.i; fl = klow.f; fh = khigh.f; fpred = kpred.f;
        /* nlopt_stop_ftol(stop, fl, fh): relstop of stop.c:81-86 with the isinf(vold) guard */
        if (cw_tol_reached(fh, fl, P.ftol_rel, P.ftol_abs)) { rc = CW_FTOL_REACHED; go = GO_DONE; break; }
        /* the centroid (nldrmd.c:195-202): lane j adds coordinate j over the points in index order, skipping high, then MULTIPLIES by
         * ninv = 1.0 / n; recomputed every iteration — an incrementally updated centroid changes the bits */
        for (int j = lane; j < n; j += CW_LANES) {
            double cj = 0.;
            for (int i = 0; i <= n; ++i) if (i != ihigh) cj += pts[(size_t) rs * i + j];
            c[j] = cj * ninv;
        }
        /* nlopt_stop_x(stop, c, xcur) with xcur = the greatest radius from the centroid (nldrmd.c:204-228).  With xtol_rel <= 0 and no
         * xtol_abs the test cannot hold (stop.c:101-103: a norm is never < 0 or < NaN), and reflectpt overwrites xcur: skipped then */
        if (P.xtol_rel > 0 || P.xtol_abs) {
            for (int j = lane; j < n; j += CW_LANES) {
                const double cj = c[j];
                double r = 0.;
                for (int i = 0; i <= n; ++i) { const double d = fabs(pts[(size_t) rs * i + j] - cj); if (d > r) r = d; }
                xcur[j] = r + cj;
            }
            /* the two weighted L1 norms (stop.c:37-79) in ascending coordinate order, whatever `exact` is */
            double dnorm = 0., xnorm = 0.;
            const double *w = P.x_weights;
            lb_seq_sum2<false>(0, n, &dnorm, &xnorm, [&](int i, double *pa, double *pb) {
                *pa = w ? w[i] * fabs(c[i] - xcur[i]) : fabs(c[i] - xcur[i]);
                *pb = w ? w[i] * fabs(c[i]) : fabs(c[i]);
            }, XB);
            int stop = dnorm < P.xtol_rel * xnorm;                /* `<` on the norms */
            if (!stop && P.xtol_abs) {
                int over = 0;
                for (int j = lane; j < n; j += CW_LANES) if (fabs(c[j] - xcur[j]) >= P.xtol_abs[j]) over = 1;      /* `>=` on the xtol_abs test */
                stop = lb_block_isum(over, S) == 0;
            }
            if (stop) { rc = CW_XTOL_REACHED; go = GO_DONE; break; }
        }
        CW_SYNC();
        if (!nm_reflect(n, xcur, c, ALPHA, pts + (size_t) rs * ihigh, lb, ub, S, lane)) { rc = CW_XTOL_REACHED; go = GO_DONE; break; }
        for (int j = lane; j < n; j += CW_LANES) xev[j] = xcur[j];
        CW_SYNC();
        stage = NM_REFLECT; go = GO_EVAL;
        break;
    }
    }
    /* X row `inst` holds the best point seen, minf its value */
    if (lane == 0) {
        out[inst].f = minf; out[inst].ret = rc; out[inst].nevals = nevals; out[inst].iterm = nevals; out[inst].cols = faildim;
        if (EXT) { E.req[inst].state = 2; E.req[inst].want_grad = 0; }
        else if (P.done) __hip_atomic_fetch_add(P.done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

#ifdef NLA_SIMT_EMU
static double nm_lds[4 * NLA_NLDRMD_MAX_N + 1];                   /* (the CPU emulation runs one workgroup at a time) */
#endif

template <int OBJ>
__global__ __launch_bounds__(CW_LANES) void nldrmd_batch_kernel(int n, int ld, int count, const double *__restrict__ lb, const double *__restrict__ ub,
                                                                const double *__restrict__ dx_given, double *__restrict__ X, double *work,
                                                                size_t slice, nla_nldrmd_params P, nla_lbfgs_result *__restrict__ out)
{
#ifndef NLA_SIMT_EMU
    extern __shared__ __attribute__((aligned(16))) double nm_lds[];
#endif
    __shared__ lb_shared S;
    __shared__ double oscratch[8];
    __shared__ lb_exact_buf XB;
    nm_search<OBJ, false>(n, ld, count, lb, ub, dx_given, X, P, out, nm_lds, work + (size_t) blockIdx.x * slice, S, oscratch, XB);
}

__global__ __launch_bounds__(CW_LANES) void nldrmd_batch_ext_kernel(int n, int ld, int count, const double *__restrict__ lb, const double *__restrict__ ub,
                                                                    const double *__restrict__ dx_given, double *__restrict__ X, double *work,
                                                                    size_t slice, nla_nldrmd_params P, nla_lbfgs_result *__restrict__ out, nla_local_ext E)
{
#ifndef NLA_SIMT_EMU
    extern __shared__ __attribute__((aligned(16))) double nm_lds[];
#endif
    __shared__ lb_shared S;
    __shared__ double oscratch[8];                   /* (the objective's buffer: this instance never touches it) */
    __shared__ lb_exact_buf XB;                      /* (the x-stop test's ordered sums) */
    nm_search<0, true>(n, ld, count, lb, ub, dx_given, X, P, out, nm_lds, work + (size_t) blockIdx.x * slice, S, oscratch, XB, E);
}

extern "C" int nla_nldrmd_serves(int n) { return n >= 1 && n <= NLA_NLDRMD_MAX_N; }
/* 16 doubles more for the launcher to start the first slice on a 128-byte boundary wherever `work` starts */
extern "C" size_t nla_nldrmd_work_doubles(int n, int count)
{
    if (!nla_nldrmd_serves(n)) return 0;
    return nm_slice_doubles(n) * (size_t) (count > 0 ? count : 1) + 16;
}
extern "C" size_t nla_nldrmd_save_bytes(int n) { return nla_nldrmd_serves(n) ? sizeof(double) * nm_save_doubles(n) : 0; }

extern "C" int nla_k_nldrmd_batch(int obj, int n, int ld, int count, const double *lb, const double *ub, const double *dx, double *X,
                                  double *work, const nla_nldrmd_params *params, nla_lbfgs_result *out, const nla_local_ext *ext, void *stream)
{
    if (count <= 0) return 0;
    if (!nla_nldrmd_serves(n) || ld < n || !lb || !ub || !X || !work || !params || !out) return (int) hipErrorInvalidValue;
    if (obj == NLA_OBJ_EXTERNAL ? (!ext || !ext->req || !ext->EX || !ext->EF || !ext->save) : (obj < 0 || ext != nullptr)) return (int) hipErrorInvalidValue;
    hipStream_t st = (hipStream_t) stream;
    nla_nldrmd_params P = *params;
    if (P.sign == 0.) P.sign = 1.;
    const size_t lds = sizeof(double) * nm_vec_doubles(n), slice = nm_slice_doubles(n);      /* (at most 8.2 KB: no attribute to raise) */
    double *base = (double *) (((uintptr_t) work + 127) & ~(uintptr_t) 127);
    if (obj == NLA_OBJ_EXTERNAL) {
        nla_local_ext E = *ext;
        P.abort = nullptr; P.done = nullptr;         /* the coroutine's stops are ext->forced / ext->timeout, its end req[].state = 2 */
        hipLaunchKernelGGL(nldrmd_batch_ext_kernel, dim3(count), dim3(CW_LANES), lds, st, n, ld, count, lb, ub, dx, X, base, slice, P, out, E);
    } else {
#define CALL(O) hipLaunchKernelGGL((nldrmd_batch_kernel<O>), dim3(count), dim3(CW_LANES), lds, st, n, ld, count, lb, ub, dx, X, base, slice, P, out)
        NLA_OBJ_DISPATCH(obj, CALL)
#undef CALL
    }
    NLA_LAUNCH_CHECK();
    return 0;
}
