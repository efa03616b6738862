/* tnewton_kernels.hip — batched NLOPT_LD_TNEWTON / _RESTART / _PRECOND / _PRECOND_RESTART (Luksan's truncated Newton PNET,
 * src/algs/luksan/pnet.c:128-564) on gfx950: one workgroup of LB_T threads per local search, the whole optimisation loop on the device,
 * as lbfgs_kernels.hip runs PLIS.
 *
 * mos = algorithm - NLOPT_LD_TNEWTON; mos1 = 1 + mos % 2 (2: steepest-descent restarts, pnet.c:340-345), mos2 = 1 + mos / 2 (2: the CG
 * iteration is preconditioned by a limited-memory BFGS matrix over mx <= mf stored pairs, pnet.c:366-384,436-449,546-553), as
 * optimize.c:733-738 derives them.
 *
 * Reference loops replaced: the inner conjugate-gradient iteration with finite-difference Hessian-vector products (pnet.c:328-469:
 * per CG step one gradient at the probe point xo + pp xs, four masked dot products and four axpys over n), the Strang recurrences
 * mxdrcb / mxdrcf of the preconditioner (mssubs.c:353-441), the bound handling pcbs04 / pyadc0 / pyrmc0 / pytrcg / pytrcs / pytrcd
 * (pssubs.c) and the objective + gradient evaluation.  The scalar control flow — PS1L01 / PNINT1 and PYFUT1 — is ../lbfgs_scalar.h with
 * PNET's constants (pnet.c:209-260: tolp = .9), executed redundantly by every thread on workgroup-uniform values.
 *
 * Storage per search: ten vectors of ld doubles in `work` (xl, xu, gf, gn, s, xo, go, xs, gs and the best point seen), ld ints in
 * `iwork`; for mos2 = 2 the 2 x mf x ld history in `hist` and 2 mf column scalars behind the vectors of `work` — column "i-th newest"
 * is ring-indexed where the reference shifts every column (mxdrsu, mssubs.c:503-524), same numbers.  mos2 = 1 is called with mf = 0 and
 * touches neither.  Any n: every vector loop is thread-strided over global memory (L2-resident at the sizes a batch has per search).
 *
 * Passes, tree-sum mode: the CG step's two axpys (s += alf xs, gs -= alf go) and the two dot products over their results are one pass;
 * the difference quotient go = (g(probe) - gn) / pp and <xs, go> are one pass.  With params.exact ("amd_exact_dot") every sum is
 * accumulated in the reference's sequential order (local_common.h) and the iterates are the reference's bit for bit (up to the device
 * libm inside a device objective).  Tree mode is NOT close to bit-comparable: the quotient divides by pp ~ 3e-8 / |xs|.
 *
 * Three evaluation points: the first point, the CG probe (its f is ignored by the algorithm), the line search.  With
 * OBJ == NLA_OBJ_EXTERNAL the kernel is a coroutine with three resume labels (include/nlopt_amd.h "External evaluation").
 *
 * The returned point: the reference wraps these four algorithms' objective in memoize_func (optimize.c:460-508,1026-1036,1064-1071) and
 * returns the best value among ALL evaluated points — probes included — that lie inside the caller's lb / ub, the first one on ties.
 * The kernel keeps that value and its point (tested against the caller's box, not xl / xu as set for fixed coordinates) and returns
 * them as x and f; a search none of whose points was inside the box returns the algorithm's own x and f.
 */
#include "local_common.h"
#include <limits.h>
#include <float.h>
#include "../lbfgs_scalar.h"
#include "luksan_bounds.h"
#include "../../../include/nlopt_amd.h"

/* scalar state of one search across an external evaluation (everything else lives in the search's vectors) */
#define TN_SCALARS(F) F(lss) F(q) F(c) F(gmax) F(umax) F(fval) F(fo) F(p) F(po) F(gnorm) F(snorm) F(rmax) F(rmin) F(rho) F(rho1) F(rho2) \
                      F(alf) F(par) F(a) F(b) F(pp) F(bestf) F(kd) F(nred) F(maxst) F(xstop) F(nevals) F(mx) F(head) F(iterd) F(cols)
struct tn_saved {
    lb_ls_state lss; lb_ls_io q; lb_counters c;
    double gmax, umax, fval, fo, p, po, gnorm, snorm, rmax, rmin, rho, rho1, rho2, alf, par, a, b, pp, bestf;
    int kd, nred, maxst, xstop, nevals, mx, head, iterd, cols, point;
};

/* a compiled-in objective: two workgroups per CU (<= 256 registers per lane), no scratch.  The coroutine keeps every scalar of the search
 * alive across its three save / load points and would spill more than the L-BFGS coroutine does under that cap (1660 bytes against
 * 1588); its time is the launches and the host's evaluations, not occupancy, so it takes the registers instead: one workgroup per CU,
 * 612 bytes of scratch (tools/kernel_resources.py) */
#ifndef TN_WAVES_PER_EU
#define TN_WAVES_PER_EU 2
#endif
#define TN_WAVES(OBJ) ((OBJ) == NLA_OBJ_EXTERNAL ? 1 : TN_WAVES_PER_EU)
template <int OBJ>
__global__ __launch_bounds__(LB_T) __attribute__((amdgpu_waves_per_eu(TN_WAVES(OBJ), TN_WAVES(OBJ)))) void tnewton_batch_kernel(
    int n, int ld, int mf, int mos, int count, const double *__restrict__ lb, const double *__restrict__ ub, double *__restrict__ X,
    double *__restrict__ work, int *__restrict__ iwork, double *__restrict__ hist, nla_lbfgs_params P, nla_lbfgs_result *__restrict__ out,
    nla_local_ext E)
{
    constexpr bool EXT = OBJ == NLA_OBJ_EXTERNAL;
    __shared__ lb_shared S;
    __shared__ double oscratch[2 * LB_W];
    __shared__ lb_exact_buf XB;
    const int inst = blockIdx.x, tid = threadIdx.x;
    if (inst >= count) return;
    if (EXT && E.resume && E.req[inst].state != 1) return;          /* finished earlier (or never asked) */
    const int mos1 = 1 + mos % 2, mos2 = 1 + mos / 2;
    double *x = X + (size_t) inst * ld;
    double *xl = work + (size_t) inst * 10 * ld, *xu = xl + ld, *gf = xu + ld, *gn = gf + ld, *s = gn + ld, *xo = s + ld, *go = xo + ld,
           *xs = go + ld, *gs = xs + ld, *bx = gs + ld;
    int *ix = iwork + (size_t) inst * ld;
    double *hx = hist + (size_t) inst * 2 * (size_t) mf * ld, *hg = hx + (size_t) mf * ld;
    double *ucol = work + (size_t) count * 10 * ld + (size_t) inst * 2 * mf, *vcol = ucol + mf;
    int head = 0;
#define COLX(i) (hx + (size_t) ((head + (i) - 1) % mf) * ld)
#define COLG(i) (hg + (size_t) ((head + (i) - 1) % mf) * ld)
#define COLU(i) (ucol[(head + (i) - 1) % mf])

    lb_ls_state lss;
    lb_ls_io q;
    lb_counters c;
    lb_stop ls;
    double gmax = 0, umax = 0, fval = 0, fo, p = 0, po = 0, a = 0, b = 0, gnorm = 0, snorm = 0, rmax, rmin = 0, rho = 0, rho1 = 0, rho2 = 0,
           alf = 0, par = 0, pp = 0, bestf = DBL_MAX, fprobe = 0;
    const double eta0 = 1e-15, eta9 = 1e120, eps = .8, eps8 = 1., eps9 = 1e-8, alf1 = 1e-10, alf2 = 1e10, told = 1e-4, xmax = 1e16, maxf = 1e20,
                 minf_est = -HUGE_VAL;
    int kd = 1, nred = 0, maxst = 0, xstop = 0, nevals = 0, mx = 0, iterd = 0, cols = 0, forced = 0, tmo = 0;
    const int mmx = n + 3;
    double xtol_rel = P.xtol_rel, tolg = P.tolg;
    tn_saved *sv = EXT ? (tn_saved *) E.save + inst : nullptr;
#define MDOT(u, v) (P.exact ? lb_mdot_exact(n, u, v, ix, XB) : lb_mdot(n, u, v, ix, S))
    /* an evaluation point: device objective -> evaluate here; external -> publish the point, save the state, leave */
#define TN_SAVE_(f) sv->f = f;
#define TN_LOAD_(f) f = sv->f;
#define TN_EVAL(POINT, LABEL, FOUT)                                                                                     \
    if (EXT) {                                                                                                          \
        for (int i = tid; i < n; i += LB_T) E.EX[(size_t) inst * ld + i] = x[i];                                        \
        if (tid == 0) {                                                                                                 \
            TN_SCALARS(TN_SAVE_)                                                                                        \
            sv->point = POINT;                                                                                          \
            E.req[inst].state = 1; E.req[inst].want_grad = 1;                                                           \
        }                                                                                                               \
        return;                                                                                                         \
    LABEL:                                                                                                              \
        for (int i = tid; i < n; i += LB_T) gf[i] = E.EG[(size_t) inst * ld + i];                                       \
        __syncthreads();                                                                                                \
        FOUT = E.EF[inst];                                                                                              \
    } else FOUT = lb_objgrad<EXT ? 0 : OBJ>(n, x, gf, S, oscratch, P.exact, XB, P.sign)
    /* behind every evaluation: memoize_func's rule (optimize.c:460-482), the f trace, the counters (pnet.c:301-302,399-400,527-528) */
    auto evaluated = [&](double fv) {
        int outside = 0;
        for (int i = tid; i < n; i += LB_T) outside += (x[i] < lb[i]) | (x[i] > ub[i]);
        if (lb_block_isum(outside, S) == 0 && fv < bestf) {
            bestf = fv;
            for (int i = tid; i < n; i += LB_T) bx[i] = x[i];
        }
        if (P.ftrace && tid == 0 && nevals < P.ftrace_cap) P.ftrace[(size_t) inst * P.ftrace_cap + nevals] = fv;
        ++nevals; ++c.nfg;
    };
    /* v := H v with the limited-memory BFGS matrix over the mx newest pairs (mxdrcb, scaling by b / a, mxdrcf: pnet.c:374-382,439-446) */
    auto precondition = [&](double *v) {
        for (int j = 1; j <= mx; ++j) {                          /* mxdrcb */
            const double *cx = COLX(j), *cg = COLG(j);
            const double d = MDOT(v, cx);
            const double w = COLU(j) * d;
            if (tid == 0) vcol[j - 1] = w;
            for (int i = tid; i < n; i += LB_T) if (ix[i] >= 0) v[i] = v[i] + (-w) * cg[i];
            __syncthreads();
        }
        if (a > 0.) { const double sc = b / a; for (int i = tid; i < n; i += LB_T) v[i] = v[i] * sc; __syncthreads(); }
        for (int j = mx; j >= 1; --j) {                          /* mxdrcf */
            const double *cx = COLX(j), *cg = COLG(j);
            const double d = MDOT(v, cg);
            const double w = vcol[j - 1] - COLU(j) * d;
            for (int i = tid; i < n; i += LB_T) if (ix[i] >= 0) v[i] = v[i] + w * cx[i];
            __syncthreads();
        }
        cols += 2 * mx;
    };

    if (xtol_rel <= 0.) xtol_rel = 1e-16;                                    /* pnet.c:241-249 */
    ls.minf_max = P.minf_max; ls.ftol_rel = P.ftol_rel <= 0. ? 1e-14 : P.ftol_rel; ls.ftol_abs = P.ftol_abs; ls.maxeval = P.maxeval;
    if (tolg <= 0.) tolg = 1e-8;
    memset(&c, 0, sizeof c);
    memset(&lss, 0, sizeof lss);
    memset(&q, 0, sizeof q);
    fo = minf_est; rmax = eta9;
    if (EXT) { forced = E.forced; tmo = E.timeout; }
    if (EXT && E.resume) {                                                   /* continue where the search left */
        TN_SCALARS(TN_LOAD_)
        __syncthreads();
        if (tid == 0) E.req[inst].state = 0;
        if (sv->point == 0) goto resume_first;
        if (sv->point == 1) goto resume_probe;
        goto resume_linesearch;
    }

    for (int i = tid; i < n; i += LB_T) {                                    /* pnet.c:614-620 */
        const int lbu = lb[i] <= -0.99 * HUGE_VAL, ubu = ub[i] >= 0.99 * HUGE_VAL;
        int t = lbu ? (ubu ? 0 : 2) : (ubu ? 1 : (lb[i] == ub[i] ? 5 : 3));
        double l = lb[i], u = ub[i];
        if ((t == 3 || t == 4) && u <= l) { u = l; t = 5; }                  /* pnet.c:284-296 */
        else if (t == 5 || t == 6) { l = x[i]; u = x[i]; t = 5; }
        ix[i] = t; xl[i] = l; xu[i] = u;
        xo[i] = 0.; go[i] = 0.; xs[i] = 0.; gs[i] = 0.; bx[i] = x[i];        /* the reference zero-fills from xo on (pnet.c:626) */
    }
    c.ites = 1; c.mtesx = 2; c.mtesf = 2; c.iters = 2; c.ires1 = 999; c.ires2 = 0; c.kd = 1;
    c.mit = INT_MAX; c.mfg = INT_MAX;                                        /* (maxeval is mfv, which pnet_ never reads: PYFUT1 tests it) */
    c.kit = -(c.ires1 * n + c.ires2);
    __syncthreads();
    lb_project(n, x, ix, xl, xu, eps9);
    __syncthreads();
    lb_add_active(n, x, ix, xl, xu);
    __syncthreads();
    TN_EVAL(0, resume_first, fval);
    evaluated(fval);
    if (!EXT && P.abort) tmo = lb_poll_abort(P.abort) == 100;
    if (tmo) c.iterm = 100;                                                  /* pnet.c:303 */

    while (c.iterm != 100) {
        /* pytrcg: largest free gradient component, largest wrong-signed multiplier on an active bound; gn := gf */
        {
            double gm = 0, um = 0;
            for (int i = tid; i < n; i += LB_T) {
                const double t = gf[i];
                const int ii = ix[i];
                gn[i] = t;
                if (ii >= 0) gm = LB_MAX(gm, fabs(t));
                else if (ii <= -5) { }
                else if (ii == -1 || ii == -3) { if (-t > um) um = -t; }
                else if (ii == -2 || ii == -4) { if (t > um) um = t; }
            }
            gmax = lb_block_max(gm, S);
            umax = lb_block_max(um, S);
        }
        c.kd = kd;
        if (!EXT && P.abort) { const int ab = lb_poll_abort(P.abort); forced = ab == -999; tmo = ab == 100; }
        lb_pyfut1(n, fval, &fo, umax, gmax, xstop, &ls, forced, nevals, tolg, &c);
        if (c.iterm != 0) break;
        if (tmo) { c.iterm = 100; break; }                                   /* pnet.c:315 */
        if (rmax > 0. && umax > eps8 * gmax) {                               /* pyrmc0: release wrong-signed active bounds */
            int rel = 0;
            for (int i = tid; i < n; i += LB_T) {
                const int t = ix[i];
                if (t >= 0 || t <= -5) continue;
                if ((t == -1 || t == -3) && -gn[i] <= 0.) continue;
                if ((t == -2 || t == -4) && gn[i] <= 0.) continue;
                ++rel;
                ix[i] = LB_MIN(-t, 3);
            }
            if (lb_block_isum(rel, S) > 1) c.irest = LB_MAX(c.irest, 1);
        }
        if (umax > eps8 * gmax) c.irest = LB_MAX(c.irest, 1);                /* pnet.c:319-321 */
        for (int i = tid; i < n; i += LB_T) xo[i] = x[i];
        __syncthreads();
    direction:
        if (c.irest != 0) {
            if (c.kit < c.nit) { mx = 0; c.kit = c.nit; }
            else { c.iterm = -10; if (c.iters < 0) c.iterm = c.iters - 5; break; }
            if (mos1 > 1) {                                                  /* steepest descent (mxvneg: every coordinate) */
                for (int i = tid; i < n; i += LB_T) s[i] = -gn[i];
                __syncthreads();
                gnorm = sqrt(MDOT(gn, gn));
                snorm = gnorm;
                goto direction_done;
            }
        }
        rho1 = MDOT(gn, gn);
        gnorm = sqrt(rho1);
        par = LB_MIN(eps, sqrt(gnorm));
        if (par > .01) par = LB_MIN(par, 1. / (double) c.nit);
        par *= par;
        /* CG initiation */
        rho = rho1; snorm = 0.;
        for (int i = tid; i < n; i += LB_T) { const double t = -gn[i]; s[i] = 0.; gs[i] = t; xs[i] = t; }
        __syncthreads();
        if (mos2 > 1) {
            b = mx == 0 ? 0. : MDOT(COLX(1), COLG(1));
            if (b > 0.) {
                if (tid == 0) COLU(1) = 1. / b;
                a = MDOT(COLG(1), COLG(1));                                  /* (mxdrcb does not touch the history: the same value) */
                precondition(xs);
            }
        }
        rho = MDOT(gs, xs);
        nred = 0;
        for (;;) {
            ++nred;
            if (nred > mmx) break;
            fo = fval;
            pp = sqrt(eta0 / MDOT(xs, xs));
            for (int i = tid; i < n; i += LB_T) if (ix[i] >= 0) x[i] = xo[i] + pp * xs[i];      /* the probe: not projected (pnet.c:395-399) */
            __syncthreads();
            TN_EVAL(1, resume_probe, fprobe);
            evaluated(fprobe);
            {
                const double ipp = 1. / pp;
                if (P.exact) {
                    for (int i = tid; i < n; i += LB_T) { const double d = gf[i] - gn[i]; go[i] = d * ipp; }
                    __syncthreads();
                    alf = MDOT(xs, go);
                } else {
                    double t = 0;
                    for (int i = tid; i < n; i += LB_T) {
                        const double d = gf[i] - gn[i], g = d * ipp;
                        go[i] = g;
                        if (ix[i] >= 0) t += xs[i] * g;
                    }
                    alf = lb_block_sum(t, S);
                }
            }
            if (alf <= 1. / eta9) {                                          /* CG fails: the matrix is not positive definite */
                if (nred == 1) {
                    for (int i = tid; i < n; i += LB_T) s[i] = -gn[i];
                    __syncthreads();
                    snorm = gnorm;
                }
                iterd = 0;
                break;
            }
            iterd = 2;
            alf = rho / alf;                                                 /* CG step */
            {
                const double nalf = -alf;
                double t1 = 0, t2 = 0;
                for (int i = tid; i < n; i += LB_T) if (ix[i] >= 0) {
                    const double sn = s[i] + alf * xs[i], gn_ = gs[i] + nalf * go[i];
                    s[i] = sn; gs[i] = gn_;
                    t1 += gn_ * gn_; t2 += sn * sn;
                }
                if (P.exact) { __syncthreads(); rho2 = MDOT(gs, gs); snorm = sqrt(MDOT(s, s)); }
                else { rho2 = lb_block_sum(t1, S); snorm = sqrt(lb_block_sum(t2, S)); }
            }
            if (rho2 <= par * rho1) break;
            if (nred >= mmx) break;
            if (mos2 > 1 && b > 0.) {
                for (int i = tid; i < n; i += LB_T) go[i] = gs[i];
                __syncthreads();
                precondition(go);
                rho2 = MDOT(gs, go);
                alf = rho2 / rho;
                for (int i = tid; i < n; i += LB_T) if (ix[i] >= 0) xs[i] = go[i] + alf * xs[i];
            } else {
                alf = rho2 / rho;
                for (int i = tid; i < n; i += LB_T) if (ix[i] >= 0) xs[i] = gs[i] + alf * xs[i];
            }
            __syncthreads();
            rho = rho2;
        }
    direction_done:
        for (int i = tid; i < n; i += LB_T) { x[i] = xo[i]; gf[i] = gn[i]; }
        __syncthreads();
        if (kd > 0) p = MDOT(gn, s);
        if (iterd < 0) c.iterm = iterd;
        else {
            if (snorm <= 0.) c.irest = LB_MAX(c.irest, 1);
            else if (p + told * gnorm * snorm <= 0.) c.irest = 0;
            else c.irest = LB_MAX(c.irest, 1);
            if (c.irest == 0) {
                nred = 0;
                rmin = alf1 * gnorm / snorm;
                rmax = LB_MIN(alf2 * gnorm / snorm, xmax / snorm);
            }
        }
        if (c.iterm != 0) break;
        if (tmo) { c.iterm = 100; break; }                                   /* pnet.c:507 */
        if (c.irest != 0) goto direction;
        /* pytrcs: save x, g in xo, go; zero s on active bounds; largest step inside the box */
        q.fp = fo; fo = fval; po = p;
        {
            double rm = rmax;
            for (int i = tid; i < n; i += LB_T) {
                xo[i] = x[i]; go[i] = gf[i];
                if (ix[i] < 0) s[i] = 0.;
                else {
                    if ((ix[i] == 1 || ix[i] >= 3) && s[i] < -1. / eta9) rm = LB_MIN(rm, (xl[i] - x[i]) / s[i]);
                    if ((ix[i] == 2 || ix[i] >= 3) && s[i] > 1. / eta9) rm = LB_MIN(rm, (xu[i] - x[i]) / s[i]);
                }
            }
            rmax = lb_block_min(rm, S);
        }
        if (rmax != 0.) {
            q.f = fval; q.fo = fo; q.p = p; q.po = po; q.minf_est = minf_est; q.maxf = maxf; q.rmin = rmin; q.rmax = rmax;
            q.tols = 1e-4; q.tolp = .9; q.kd = kd; q.ld = -1; q.nit = c.nit; q.kit = c.kit; q.nred = nred; q.mred = 10;
            q.maxst = maxst; q.iest = 0; q.inits = 2; q.iters = c.iters; q.kters = 3; q.mes = 4; q.isys = 0;
            for (;;) {
                lb_ps1l01(&q, &lss);
                if (q.isys == 0) break;
                for (int i = tid; i < n; i += LB_T) if (ix[i] >= 0) x[i] = xo[i] + q.r * s[i];
                __syncthreads();
                lb_project(n, x, ix, xl, xu, eps9);
                __syncthreads();
                TN_EVAL(2, resume_linesearch, q.f);
                evaluated(q.f);
                q.p = MDOT(gf, s);
            }
            fval = q.f; p = q.p; kd = q.kd; nred = q.nred; maxst = q.maxst; c.iters = q.iters;
            if (c.iters <= 0) {                                              /* zero step: restore and restart */
                fval = fo; p = po;
                for (int i = tid; i < n; i += LB_T) { x[i] = xo[i]; gf[i] = go[i]; }
                __syncthreads();
                c.irest = LB_MAX(c.irest, 1);
                goto direction;
            }
            /* pytrcd: xo, go := differences (zero on active coordinates); nlopt_stop_dx(x, dx) */
            {
                double nx = 0, ndx = 0;
                for (int i = tid; i < n; i += LB_T) {
                    double ddx = x[i] - xo[i], ddg = gf[i] - go[i];
                    if (ix[i] < 0) { ddx = 0.; ddg = 0.; }
                    xo[i] = ddx; go[i] = ddg;
                    if (P.x_weights) { nx += P.x_weights[i] * fabs(x[i]); ndx += P.x_weights[i] * fabs(ddx); }
                    else { nx += fabs(x[i]); ndx += fabs(ddx); }
                }
                po = q.r * po; p = q.r * p;
                if (P.exact) {                                                /* stop.c:37-57 vector_norm, sequential */
                    __syncthreads();
                    const double *w = P.x_weights;
                    nx = lb_seq_sum(n, 0., [&](int i) { return w ? w[i] * fabs(x[i]) : fabs(x[i]); }, XB.a);
                    ndx = lb_seq_sum(n, 0., [&](int i) { return w ? w[i] * fabs(xo[i]) : fabs(xo[i]); }, XB.a);
                } else {
                    nx = lb_block_sum(nx, S);
                    ndx = lb_block_sum(ndx, S);
                }
                xstop = ndx < xtol_rel * nx;                                  /* nlopt_stop_dx, stop.c:110-120 */
                if (!xstop && P.xtol_abs) {
                    int viol = 0;
                    __syncthreads();
                    for (int i = tid; i < n; i += LB_T) viol += fabs(xo[i]) >= P.xtol_abs[i];
                    xstop = lb_block_isum(viol, S) == 0;
                }
            }
            if (mos2 > 1) {                                                   /* pnet.c:546-553: the pair becomes the newest column */
                /* mxdrsu copies u(i) to u(i + 1) and leaves u(1) as it was: where the next direction finds b <= 0 and does not set it, the
                 * column behind inherits it */
                const double u1 = COLU(1);
                mx = LB_MIN(mx + 1, mf);
                __syncthreads();
                head = (head + mf - 1) % mf;
                double *cx = COLX(1), *cg = COLG(1);
                if (tid == 0) COLU(1) = u1;
                for (int i = tid; i < n; i += LB_T) { cx[i] = xo[i]; cg[i] = go[i]; }
            }
        }
        __syncthreads();
        {
            const int inew = lb_block_isum(lb_add_active_count(n, x, ix, xl, xu), S);   /* pyadc0 */
            if (inew > 0) c.irest = LB_MAX(c.irest, 1);
        }
        __syncthreads();
    }
    __syncthreads();
    if (bestf < DBL_MAX) { for (int i = tid; i < n; i += LB_T) x[i] = bx[i]; fval = bestf; }
    if (tid == 0) {
        out[inst].f = fval; out[inst].ret = lb_result_of_iterm(c.iterm); out[inst].nevals = nevals; out[inst].iterm = c.iterm; out[inst].cols = cols;
        if (P.done) __hip_atomic_fetch_add(P.done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (EXT) E.req[inst].state = 2;
    }
#undef MDOT
#undef TN_EVAL
#undef TN_SAVE_
#undef TN_LOAD_
#undef COLX
#undef COLG
#undef COLU
}

extern "C" size_t nla_tnewton_work_doubles(int ld, int mf, int count) { return (size_t) count * (10 * (size_t) ld + 2 * (size_t) mf); }
extern "C" size_t nla_tnewton_hist_doubles(int ld, int mf, int count) { return (size_t) count * 2 * (size_t) mf * (size_t) ld; }
extern "C" size_t nla_tnewton_save_bytes(void) { return sizeof(tn_saved); }

extern "C" int nla_k_tnewton_batch(int obj, int n, int ld, int mf, int mos, int count, const double *lb, const double *ub, double *X,
                                   double *work, int *iwork, double *hist, const nla_lbfgs_params *params, nla_lbfgs_result *out,
                                   const nla_local_ext *ext, void *stream)
{
    if (count <= 0) return 0;
    if (n < 1 || ld < n || mos < 0 || mos > 3 || !lb || !ub || !X || !work || !iwork || !params || !out) return (int) hipErrorInvalidValue;
    if (mos >= 2 ? (mf < 1 || !hist) : mf != 0) return (int) hipErrorInvalidValue;       /* (mos2 = 1 keeps no history) */
    hipStream_t st = (hipStream_t) stream;
    nla_lbfgs_params P = *params;
    nla_local_ext E = {};
    if (P.sign == 0.) P.sign = 1.;
    P.exact = P.exact & 1;
    if (obj == NLA_OBJ_EXTERNAL) {
        if (!ext || !ext->req || !ext->EX || !ext->EG || !ext->EF || !ext->save) return (int) hipErrorInvalidValue;
        E = *ext;
    }
#define CALL(O) hipLaunchKernelGGL((tnewton_batch_kernel<O>), dim3(count), dim3(LB_T), 0, st, n, ld, mf, mos, count, lb, ub, X, work, iwork, hist, P, out, E)
    if (obj == NLA_OBJ_EXTERNAL) { CALL(NLA_OBJ_EXTERNAL); }
    else NLA_OBJ_DISPATCH(obj, CALL)
#undef CALL
    NLA_LAUNCH_CHECK();
    return 0;
}
