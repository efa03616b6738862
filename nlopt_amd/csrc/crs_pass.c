/* crs_pass.c — what the CRS2_LM engine (crs_engine.h) puts on the main stream per pass: the conservative pass (ops->advance) in its three
 * transports — column-sharded, lists as kernel arguments, lists by upload — and the device-resolved window (ops->chain), single-device
 * and column-sharded.  Every transport is one function; the dispatchers in front of them and the epilogues behind them are shared. */
#include "crs_engine.h"

#define TIME_EVERY 8                       /* conservative passes below n = 2048: one in so many is timed */
#define TIME_EVERY_WINDOW 4                /* device-resolved windows below n = 2048 likewise */

/* one of the event pair around a pass's gather (timed passes only) */
#define EVREC(e, ev) do { if ((e)->timed) CK(e, nla_event_record((ev), (e)->main)); } while (0)
/* the sharded pass, which holds the flag `lerr`: a failure that is remembered in it and told to the other ranks in band, and one after
 * which this rank cannot take part in the exchange any more */
#define SOFT(e, lerr, call) do { if (!(lerr)) { int rc_ = (call); if (rc_) { (lerr) = 1; snprintf((e)->err, sizeof (e)->err, "%.160s failed: %s", #call, nla_dev_error_string(rc_)); } } } while (0)
#define HARD(e, lerr, call) do { int rc_ = (call); if (rc_) { if (!(lerr)) snprintf((e)->err, sizeof (e)->err, "%.160s failed: %s", #call, nla_dev_error_string(rc_)); nla_comm_abort((e)->comm); return -1; } } while (0)

/* the pass's lists through the pinned upload buffer: pieces appended one behind the other — the 8-byte arrays before the 4-byte ones, so
 * that every piece stays naturally aligned — then ONE H2D of the total.  up_add appends `bytes` from src behind the *total packed so far
 * (nothing: bytes == 0) and says where the piece will lie on the device */
static const void *up_add(nla_crs_hip_engine *e, size_t *total, const void *src, size_t bytes)
{
    const size_t at = *total;
    if (bytes) memcpy(e->h_up + at, src, bytes);
    *total += bytes;
    return e->d_up + at;
}
static int up_send(nla_crs_hip_engine *e, size_t total) { return nla_memcpy_h2d(e->d_up, e->h_up, total, e->main); }

/* the event pair of a timed pass into the statistics; the kernel's milliseconds */
static float stats_add_gather(nla_crs_hip_engine *e)
{
    const float ms = nla_event_elapsed_ms(e->ev0, e->ev1);
    if (ms >= 0) e->stats->t_gather_ms += ms;
    e->stats->gather_launches += 1;
    return ms;
}

/* upload W / t_in of the coming pass (K may be 0: commits only) together with the staged commits
 * in ONE copy, and write the commits to X before anything else runs on the main stream.
 * The pinned upload buffer is rewritten by the next pass: callers that do not synchronise
 * themselves must do so before the host touches it again (every pass ends with a sync) */
static int upload_and_commit(nla_crs_hip_engine *e, const int64_t *W, int nW, const int32_t *t_in, int K, const int64_t **d_W, const int32_t **d_tin)
{
    const int nc = e->npending;
    size_t up = 0;
    const int64_t *dW = (const int64_t *) up_add(e, &up, W, 8 * (size_t) nW), *drow = (const int64_t *) up_add(e, &up, e->pend_row, 8 * (size_t) nc);
    const int32_t *dtin = (const int32_t *) up_add(e, &up, t_in, 4 * (size_t) K);
    const int32_t *dslot = (const int32_t *) up_add(e, &up, e->pend_slot, 4 * (size_t) nc), *dkind = (const int32_t *) up_add(e, &up, e->pend_kind, 4 * (size_t) nc);
    if (up == 0) return 0;
    CK(e, up_send(e, up));
    if (nc) {
        CK(e, nla_k_crs_commit(e->nc, e->ld, e->d_X, e->d_TX, e->d_TM, nc, dslot, dkind, drow, e->main));
        e->npending = 0;
    }
    if (d_W) *d_W = dW;
    if (d_tin) *d_tin = dtin;
    return 0;
}

/* window mode: the staged commits (whole points -> rows of the slice), in launches of at most NLA_KARG_MAX; the first one also clears
 * `zero` and refreshes the whole best row from a slot */
static int commit_sh(nla_crs_hip_engine *e, void *zero, size_t zero_bytes, int best_slot, int best_kind)
{
    int done = 0, first = 1;
    while (first || done < e->npending) {
        const int cnt = e->npending - done < NLA_KARG_MAX ? e->npending - done : NLA_KARG_MAX;
        CK(e, nla_k_crs_commit_sh(e->nc, e->ld, e->ldf, e->c0, e->d_X, e->d_TX, e->d_TM, cnt, e->pend_slot + done, e->pend_kind + done, e->pend_row + done,
                                  first ? zero : NULL, first ? zero_bytes : 0, e->n, first ? best_slot : -1, best_kind, e->d_xbest, e->main));
        done += cnt; first = 0;
    }
    e->npending = 0;
    return 0;
}

int nla_crs_eng_flush_commits(nla_crs_hip_engine *e)
{
    if (!e->npending) return 0;
    if (e->shchain ? commit_sh(e, NULL, 0, -1, 0) : upload_and_commit(e, NULL, 0, NULL, 0, NULL, NULL)) return -1;
    CK(e, nla_stream_sync(e->main));
    return 0;
}

/* ---- the conservative pass ----------------------------------------------------------------------------------------------------------- */
/* spin until the finish kernel's doorbell shows `seq` (1: it did not within 20 ms — the caller synchronises the stream instead) */
static int bell_wait(nla_crs_hip_engine *e, uint32_t seq)
{
    unsigned spins = 0;
    double t0 = 0;
    while (__atomic_load_n(e->h_bell, __ATOMIC_ACQUIRE) != seq) {
#if defined(__x86_64__) || defined(__i386__)
        __builtin_ia32_pause();
#endif
        if ((++spins & 4095u) == 0) {
            const double t = nla_seconds();
            if (t0 == 0) t0 = t;
            else if (t - t0 > 0.02) return 1;
        }
    }
    return 0;
}

/* the K status records from the device into pinned memory, the driver's host work beside the pass, the wait */
static int status_copy_back(nla_crs_hip_engine *e, int K)
{
    CK(e, nla_memcpy_d2h(e->h_status, e->d_status, sizeof(nla_crs_slot_status) * (size_t) K, e->main));
    if (e->idle_fn) e->idle_fn(e->idle_arg);
    CK(e, nla_stream_sync(e->main));
    return 0;
}

/* one rank of a column-sharded run: the same pass on the slice; the slices of the candidates that completed (trial point and
 * mutation) are all-gathered and every rank evaluates the assembled points — identical status records on every rank */
static int pass_sharded(nla_crs_hip_engine *e, uint64_t first_block, int K, int64_t i0, const int64_t *W, int nW, const int32_t *t_in)
{
    const int n = e->n;
    const uint32_t ring = 2u * (uint32_t) e->B;
    const int ncol = (e->ld % 2 == 0 && e->nc % 2 != 0) ? e->nc + 1 : e->nc;      /* (an even count lets the gather take coordinate pairs; the pad column is zero) */
    const int64_t *d_W = NULL; const int32_t *d_tin = NULL;
    /* A failure on this rank alone must not leave the others waiting in the all-gather: it is REMEMBERED, the rank still packs
     * (whatever its slots hold) and joins the exchange with the value 2 in its first flag word, and every rank — this one
     * included — sees it in record K and leaves the pass with the same error.  Only a rank that cannot even pack and send gives
     * up out of band (nla_comm_abort: the shm transport's barriers fail; the other transports have no such channel). */
    int lerr = 0;
    if (upload_and_commit(e, W, nW, t_in, K, &d_W, &d_tin)) { lerr = 1; d_tin = e->d_tout; }      /* (message set; any device array of K ints serves the pack) */
    if (nla_dbg_int("NLA_CRS_FAIL_RANK", -1) == e->rank && (int64_t) e->pass_no == (int64_t) nla_dbg_int("NLA_CRS_FAIL_PASS", -1)) {
        lerr = 1; snprintf(e->err, sizeof e->err, "injected failure (NLA_CRS_FAIL_RANK / NLA_CRS_FAIL_PASS)");
    }
    EVREC(e, e->ev0);
    SOFT(e, lerr, nla_k_crs_advance_cols(n, ncol, e->ld, e->d_X, i0, e->d_jn, e->d_pos, e->d_last, ring, first_block, K, d_W, nW,
                                   d_tin, e->d_tout, KCAP - 1, e->d_lb, e->d_ub, e->d_TX, 0 /* automatic tiling */, e->main));
    EVREC(e, e->ev1);
    HARD(e, lerr, nla_k_crs_sh_mutate_pack(n, e->c0, e->nc, e->ld, e->colper, e->d_X, i0, e->d_TX, e->d_TM, e->d_words, ring, first_block, K,
                                     d_tin, e->d_tout, KCAP - 1, e->d_lb, e->d_ub, e->d_csend, lerr ? 2 : e->stop_in[0], e->stop_in[1], e->main));
    if (nla_comm_allgather_dev(e->comm, e->d_csend, e->d_crecv, sizeof(double) * (2 * (size_t) K * (size_t) e->colper + 2), e->main)) {
        nla_comm_abort(e->comm);
        if (!lerr) snprintf(e->err, sizeof e->err, "all-gather of the candidates failed: %s", nlopt_amd_comm_error(e->comm));
        return -1;
    }
    HARD(e, lerr, nla_k_crs_sh_eval(OBJK(e), n, e->colper, first_block, K, d_tin, e->d_tout, KCAP - 1, e->d_crecv, e->world, e->d_fT, e->d_fM, e->d_status, e->main));
    if (e->stats) e->stats->allgather_bytes += (uint64_t) e->world * (2 * (uint64_t) K * (uint64_t) e->colper + 2) * sizeof(double);
    /* the K status records and, behind them, the ranks' agreed stop flags (and whether any rank failed) */
    HARD(e, lerr, nla_memcpy_d2h(e->h_status, e->d_status, sizeof(nla_crs_slot_status) * ((size_t) K + 1), e->main));
    if (e->idle_fn) e->idle_fn(e->idle_arg);
    HARD(e, lerr, nla_stream_sync(e->main));
    if (e->h_status[K].t != 0) { if (!lerr) snprintf(e->err, sizeof e->err, "another rank failed in the middle of a sharded pass"); return -1; }
    e->stop_out[0] = e->h_status[K].fT != 0.; e->stop_out[1] = e->h_status[K].fM != 0.;
    return 0;
}

/* small lists (the usual case): W, the resume points and the staged commits travel as kernel arguments — no copy in
 * front of the pass */
static int pass_kargs(nla_crs_hip_engine *e, uint64_t first_block, int K, int64_t i0, const int64_t *W, int nW, const int32_t *t_in)
{
    const int n = e->n;
    const uint32_t ring = 2u * (uint32_t) e->B;
    /* the staged commits ride in the advance launch (hip/crs_kernels.hip, crs_fwd: copied by extra workgroups, reads of those rows
     * forwarded to the slots they come from) unless one of their source slots is a slot of this pass's own window — the ring
     * wrapped onto it — or there are too many: then the commit launch of its own in front, as before
     * (measured against that launch for every pass: profiles/r04_crs_fuse_commit_ab.txt) */
    int fuse = e->npending > 0 && e->npending <= NLA_KC_MAX;
    for (int c = 0; fuse && c < e->npending; ++c)
        for (int a = 0; a < K; ++a)
            if ((int32_t) ((first_block + (uint64_t) a) & (KCAP - 1)) == e->pend_slot[c]) { fuse = 0; break; }
    if (e->npending && !fuse) {
        CK(e, nla_k_crs_commit_args(n, e->ld, e->d_X, e->d_TX, e->d_TM, e->npending, e->pend_slot, e->pend_kind, e->pend_row, e->main));
        e->npending = 0;
    }
    EVREC(e, e->ev0);
    if (fuse) {
        CK(e, nla_k_crs_advance_commit_args(n, e->ld, e->d_X, i0, e->d_jn, e->d_pos, e->d_last, ring, first_block, K, W, nW,
                                            t_in, e->d_tout, KCAP - 1, e->d_lb, e->d_ub, e->d_TX, e->d_TM, e->npending, e->pend_slot,
                                            e->pend_kind, e->pend_row, 0 /* automatic tiling */, e->main));
        e->npending = 0;
    } else
        CK(e, nla_k_crs_advance_args(n, e->ld, e->d_X, i0, e->d_jn, e->d_pos, e->d_last, ring, first_block, K, W, nW,
                                     t_in, e->d_tout, KCAP - 1, e->d_lb, e->d_ub, e->d_TX, 0 /* automatic tiling */, e->main));
    EVREC(e, e->ev1);
    if (e->direct_status) {
        /* the finish kernel writes the K records straight into the pinned host buffer and rings: the pass is over for the host
         * when the bell shows this pass's number — no copy-back, no stream synchronisation (its wake-up is a third of a 30 us pass
         * at n = 512; profiles/r04_crs_doorbell_ab.txt); a bell that does not come within 20 ms falls back to the synchronisation,
         * which reports what happened */
        const uint32_t seq = ++e->bell_seq ? e->bell_seq : ++e->bell_seq;
        CK(e, nla_k_crs_finish_args_bell(OBJK(e), n, e->ld, e->d_X, i0, e->d_TX, e->d_TM, e->d_words, ring, first_block, K,
                                         t_in, e->d_tout, KCAP - 1, e->d_lb, e->d_ub, e->d_fT, e->d_fM, e->h_status, e->d_bellcount,
                                         e->h_bell, seq, e->main));
        if (e->idle_fn) e->idle_fn(e->idle_arg);
        if (bell_wait(e, seq)) CK(e, nla_stream_sync(e->main));
        return 0;
    }
    CK(e, nla_k_crs_finish_args(OBJK(e), n, e->ld, e->d_X, i0, e->d_TX, e->d_TM, e->d_words, ring, first_block, K,
                                t_in, e->d_tout, KCAP - 1, e->d_lb, e->d_ub, e->d_fT, e->d_fM, e->d_status, e->main));
    return status_copy_back(e, K);
}

/* the objective is the user's kernel: f of every window slot's trial point and mutation in two launches over the slot
 * rows (rows of unfinished slots hold partial sums: their values are never looked at), then the rings come back */
static int userobj_eval_slots(nla_crs_hip_engine *e, uint64_t first_block, int K)
{
    for (int a = 0; a < K; ++a) e->h_list[a] = -(int32_t) (((first_block + (uint64_t) a) & (KCAP - 1)) + 1);
    CK(e, nla_memcpy_h2d(e->d_list, e->h_list, sizeof(int32_t) * (size_t) K, e->main));
    CK(e, nla_userobj_evalgrad_list(e->user, e->n, e->ld, K, e->d_list, e->d_TX, e->d_fT, NULL, e->sign, e->main));
    CK(e, nla_userobj_evalgrad_list(e->user, e->n, e->ld, K, e->d_list, e->d_TM, e->d_fM, NULL, e->sign, e->main));
    CK(e, nla_memcpy_d2h(e->h_fTM, e->d_fT, sizeof(double) * 2 * KCAP, e->main));
    return 0;
}

/* long lists, the user's kernel, NLA_CRS_UPLOAD: the lists and the staged commits in one copy in front of the pass */
static int pass_upload(nla_crs_hip_engine *e, uint64_t first_block, int K, int64_t i0, const int64_t *W, int nW, const int32_t *t_in)
{
    const int n = e->n;
    const uint32_t ring = 2u * (uint32_t) e->B;
    const int64_t *d_W = NULL; const int32_t *d_tin = NULL;
    if (upload_and_commit(e, W, nW, t_in, K, &d_W, &d_tin)) return -1;
    EVREC(e, e->ev0);
    CK(e, nla_k_crs_advance(n, e->ld, e->d_X, i0, e->d_jn, e->d_pos, e->d_last, ring, first_block, K, d_W, nW,
                            d_tin, e->d_tout, KCAP - 1, e->d_lb, e->d_ub, e->d_TX, 0 /* automatic tiling */, e->main));
    EVREC(e, e->ev1);
    CK(e, nla_k_crs_finish(OBJK(e), n, e->ld, e->d_X, i0, e->d_TX, e->d_TM, e->d_words, ring, first_block, K,
                           d_tin, e->d_tout, KCAP - 1, e->d_lb, e->d_ub, e->d_fT, e->d_fM, e->d_status, e->main));
    if (e->obj == -2 && userobj_eval_slots(e, first_block, K)) return -1;
    if (status_copy_back(e, K)) return -1;
    for (int a = 0; e->obj == -2 && a < K; ++a) {
        const size_t q = (size_t) ((first_block + (uint64_t) a) & (KCAP - 1));
        e->h_status[a].fT = e->h_fTM[q]; e->h_status[a].fM = e->h_fTM[KCAP + q];
    }
    return 0;
}

/* behind every transport: the records out of pinned memory, the slots' resume points, statistics, the pass log */
static void pass_epilogue(nla_crs_hip_engine *e, uint64_t first_block, int K, int nW, const int32_t *t_in, nla_crs_slot_status *status)
{
    memcpy(status, e->h_status, sizeof(nla_crs_slot_status) * (size_t) K);
    for (int a = 0; a < K; ++a) e->h_t[(first_block + (uint64_t) a) & (KCAP - 1)] = status[a].t;
    if (e->timed) stats_add_gather(e);
    if (e->pass_log) {             /* K, nW, slots already complete / fresh / stopped short, rows summed, kernel ms */
        long rows = 0;
        int done_in = 0, fresh = 0, stopped = 0;
        for (int a = 0; a < K; ++a) {
            rows += status[a].t - t_in[a]; stopped += status[a].t < e->n;
            done_in += t_in[a] == e->n; fresh += t_in[a] == 0;
        }
        fprintf(e->pass_log, "%d,%d,%d,%d,%d,%d,%ld,%.4f\n", e->n, K, nW, done_in, fresh, stopped, rows, (double) nla_event_elapsed_ms(e->ev0, e->ev1));
    }
}

int nla_crs_eng_advance(void *ve, uint64_t first_block, int K, uint64_t fresh_from, int64_t i0, const int64_t *W, int nW, nla_crs_slot_status *status)
{
    nla_crs_hip_engine *e = (nla_crs_hip_engine *) ve;
    int32_t t_in[KCAP];
    int rc;
    if (K < 1 || K > KCAP || nW > KCAP || nW < 0) FAIL(e, "bad window K=%d nW=%d", K, nW);
    if (e->shchain) FAIL(e, "this engine was set up for device-resolved windows on a column-sharded population: no conservative passes");
    if (K > nla_crs_eng_max_slots(ve, first_block)) FAIL(e, "window reaches past the prepared batches");
    if (nla_crs_eng_ensure_blocks(e, first_block, first_block + (uint64_t) K)) { if (!e->err[0]) snprintf(e->err, sizeof e->err, "batch preparation failed"); return -1; }
    for (int a = 0; a < K; ++a) t_in[a] = first_block + (uint64_t) a >= fresh_from ? 0 : e->h_t[(first_block + (uint64_t) a) & (KCAP - 1)];
    e->timed = (e->n >= 2048 || e->pass_log || (e->pass_no++ % TIME_EVERY) == 0) && e->stats;
    if (e->sharded) rc = pass_sharded(e, first_block, K, i0, W, nW, t_in);
    else if (K <= NLA_KARG_MAX && nW <= NLA_KARG_MAX && e->npending <= NLA_KARG_MAX && !e->force_upload && e->obj != -2)
        rc = pass_kargs(e, first_block, K, i0, W, nW, t_in);
    else rc = pass_upload(e, first_block, K, i0, W, nW, t_in);
    if (rc) return -1;
    pass_epilogue(e, first_block, K, nW, t_in, status);
    return 0;
}

/* ---- the device-resolved window ------------------------------------------------------------------------------------------------------ */
/* what a launch in front of the window clears of the control block (all but its first word) */
static void *ctrl_clear_range(const nla_crs_hip_engine *e, int K, int nW, size_t *bytes)
{
    *bytes = nla_crs_chain_ctrl_bytes(K, nW) - sizeof(uint32_t);
    return (char *) e->d_ctrl + sizeof(uint32_t);
}

/* a whole window in one launch with the chain resolved on the device (hip/crs_chain.hip): commits, lists and the launch */
static int window_launch(nla_crs_hip_engine *e, uint64_t first_block, int K, int64_t i0, double f_best, const int64_t *W, const double *Wf, int nW, int fwcap)
{
    const int n = e->n;
    const uint32_t ring = 2u * (uint32_t) e->B;
    const int on_host = nW <= NLA_KARG_MAX && !e->force_upload;
    const int64_t *d_W = W; const double *d_Wf = Wf;
    /* what goes in front of the window on the stream (round 5, "lean windows": a 256-slot window used to be copy / commit / copy / fill /
     * fill / chain — six operations with 4-7 us between any two, profiles/r05_n512_timeline.txt): ONE copy with everything the device
     * needs (W, its f values, the commit lists — none at all when they fit the kernel arguments), the commit kernel of the previous
     * window's accepted points, which also clears the control block, then the window */
    size_t zero_bytes;
    void *zero = ctrl_clear_range(e, K, nW, &zero_bytes);
    int zeroed = 0, rc;
    if (e->npending && e->npending <= NLA_KARG_MAX && !e->force_upload) {
        CK(e, nla_k_crs_commit_zero(n, e->ld, e->d_X, e->d_TX, e->d_TM, e->npending, e->pend_slot, e->pend_kind, e->pend_row, 1, zero, zero_bytes, e->main));
        e->npending = 0; zeroed = 1;
    }
    if (e->npending || !on_host) {
        const int nc = e->npending, nWu = on_host ? 0 : nW;
        size_t up = 0;
        const int64_t *dW = (const int64_t *) up_add(e, &up, W, 8 * (size_t) nWu);
        const double *dWf = (const double *) up_add(e, &up, Wf, 8 * (size_t) nWu);
        const int64_t *drow = (const int64_t *) up_add(e, &up, e->pend_row, 8 * (size_t) nc);
        const int32_t *dslot = (const int32_t *) up_add(e, &up, e->pend_slot, 4 * (size_t) nc), *dkind = (const int32_t *) up_add(e, &up, e->pend_kind, 4 * (size_t) nc);
        CK(e, up_send(e, up));
        if (nc) {
            CK(e, nla_k_crs_commit_zero(e->nc, e->ld, e->d_X, e->d_TX, e->d_TM, nc, dslot, dkind, drow, 0, zero, zero_bytes, e->main));
            e->npending = 0; zeroed = 1;
        }
        if (nWu) { d_W = dW; d_Wf = dWf; }
    }
    /* the event pair around the launch (the roofline figure of bench.py) on every window from n = 2048 on, on one window in
     * TIME_EVERY_WINDOW below: two barrier packets and an elapsed-time query per ~200 us window are a few per cent there */
    e->timed = (n >= 2048 || e->pass_log || (e->pass_no++ % TIME_EVERY_WINDOW) == 0) && e->stats;
    EVREC(e, e->ev0);
    rc = nla_k_crs_chain_lean(OBJK(e), n, e->ld, e->d_X, i0, f_best, e->d_jn, e->d_pos, e->d_last, e->d_words, ring, first_block, K, d_W,
                              d_Wf, nW, on_host, KCAP - 1, e->d_lb, e->d_ub, e->d_TX, e->d_TM, e->d_ctrl, e->ticket_base, e->h_status,
                              e->h_fwcnt, e->h_fwrec, fwcap, zeroed, e->main);
    if (rc) FAIL(e, "nla_k_crs_chain failed: %s", nla_dev_error_string(rc));
    e->ticket_base += nla_crs_chain_tickets(n, e->ld, K);
    return 0;
}

/* a whole window of a column-sharded population, resolved on the device: no collective call — the slices travel inside the launch */
static int window_launch_sh(nla_crs_hip_engine *e, uint64_t first_block, int K, int64_t i0, double f_best, const int64_t *W, const double *Wf, int nW, int fwcap)
{
    const int n = e->n;
    const uint32_t ring = 2u * (uint32_t) e->B;
    const int on_host = nW <= NLA_KARG_MAX;
    const int64_t *d_W = W; const double *d_Wf = Wf;
    size_t zero_bytes;
    void *zero = ctrl_clear_range(e, K, nW, &zero_bytes);
    int best_slot = -1, best_kind = 0, rc;
    /* the whole best row: every trial starts from it (the slice in X serves that), every mutation is formed around it (that needs all of
     * it).  A new best point is an accepted trial point or mutation of the window before — whole in this rank's TX / TM, named by the
     * staged commits; only the first window's best (a row of the initial population) has to be put together from the ranks' slices
     * (as the engine's gather_point does for the host, with its own failure rules: here only the collective's failure is told to the
     * other ranks out of band) */
    if (i0 != e->xbest_row) {
        for (int c = e->npending - 1; c >= 0; --c)
            if (e->pend_row[c] == i0) { best_slot = e->pend_slot[c]; best_kind = e->pend_kind[c]; break; }
        if (best_slot < 0) {
            if (nla_crs_eng_flush_commits(e)) return -1;
            CK(e, nla_memcpy_d2d(e->d_gsend, e->d_X + (size_t) i0 * (size_t) e->ld, sizeof(double) * (size_t) e->nc, e->main));
            if (nla_comm_allgather_dev(e->comm, e->d_gsend, e->d_grecv, sizeof(double) * (size_t) e->colper, e->main)) {
                nla_comm_abort(e->comm);
                FAIL(e, "all-gather of the best row's slices failed: %s", nlopt_amd_comm_error(e->comm));
            }
            CK(e, nla_memcpy_d2d(e->d_xbest, e->d_grecv, sizeof(double) * (size_t) n, e->main));     /* (rank r's colper columns sit at r * colper = c0 of rank r) */
        }
        e->xbest_row = i0;
    }
    if (!on_host) {
        size_t up = 0;
        d_W = (const int64_t *) up_add(e, &up, W, 8 * (size_t) nW); d_Wf = (const double *) up_add(e, &up, Wf, 8 * (size_t) nW);
        CK(e, up_send(e, up));
    }
    if (commit_sh(e, zero, zero_bytes, best_slot, best_kind)) return -1;
    e->timed = e->stats != NULL;
    EVREC(e, e->ev0);
    ++e->sh_seq;
    rc = nla_k_crs_chain_sh(OBJK(e), n, e->ncolp, e->ld, e->ldf, e->d_X, i0, f_best, e->d_jn, e->d_pos, e->d_last, e->d_words, ring, first_block, K,
                            d_W, d_Wf, nW, on_host, KCAP - 1, e->d_lb, e->d_ub, e->d_TX, e->d_TM, e->d_ctrl, e->ticket_base, e->h_status,
                            e->h_fwcnt, e->h_fwrec, fwcap, 1, e->d_table, e->sh_seq, (uint32_t) ((e->stop_in[0] ? 1 : 0) | (e->stop_in[1] ? 2 : 0)), e->sh_grid_cap, e->main);
    if (rc) FAIL(e, "nla_k_crs_chain_sh failed: %s", nla_dev_error_string(rc));
    e->ticket_base += nla_crs_chain_sh_tickets(n, e->ncolp, K, e->sh_grid_cap);
    return 0;
}

/* behind either window: status and records out of pinned memory, the slots' resume points, statistics, the pass log */
static void window_epilogue(nla_crs_hip_engine *e, uint64_t first_block, int K, int nW, nla_crs_slot_status *status, uint32_t *fwcnt, uint32_t *fwrec, int fwcap)
{
    memcpy(status, e->h_status, sizeof(nla_crs_slot_status) * (size_t) K);
    memcpy(fwcnt, e->h_fwcnt, sizeof(uint32_t) * (size_t) K);
    /* only the records a slot wrote (most slots of a window read none or one of the window's worst rows): the buffer is pinned memory the
     * device has just written — every line of it is a miss for the host — and the driver reads fwrec[a][0 .. min(fwcnt[a], fwcap)) only */
    for (int a = 0; a < K; ++a) {
        const uint32_t c = e->h_fwcnt[a] < (uint32_t) fwcap ? e->h_fwcnt[a] : (uint32_t) fwcap;
        if (c) memcpy(fwrec + (size_t) a * (size_t) fwcap, e->h_fwrec + (size_t) a * (size_t) fwcap, sizeof(uint32_t) * (size_t) c);
    }
    for (int a = 0; a < K; ++a) e->h_t[(first_block + (uint64_t) a) & (KCAP - 1)] = e->n;
    if (e->timed) {
        const float ms = stats_add_gather(e);
        /* a sharded window: what this rank pushed to the others inside the launch — its columns of every slot, to world - 1 ranks */
        if (e->shchain) e->stats->allgather_bytes += (uint64_t) K * (uint64_t) (e->world - 1) * (uint64_t) e->ncolp * sizeof(double);
        if (e->pass_log) fprintf(e->pass_log, "%d,%d,%d,%d,%d,%d,%ld,%.4f\n", e->n, K, nW, 0, K, 0, (long) K * e->n, (double) ms);
    }
}

int nla_crs_eng_chain(void *ve, uint64_t first_block, int K, int64_t i0, double f_best, const int64_t *W, const double *Wf, int nW,
                      nla_crs_slot_status *status, uint32_t *fwcnt, uint32_t *fwrec, int fwcap)
{
    nla_crs_hip_engine *e = (nla_crs_hip_engine *) ve;
    if (e->obj < 0 || !e->d_ctrl) FAIL(e, "no device-resolved windows for a host objective");
    if (K < 1 || K > CHAIN_KMAX || nW < 0 || nW > CHAIN_KMAX || fwcap != CHAIN_FWCAP) FAIL(e, "bad window K=%d nW=%d", K, nW);
    if (K > nla_crs_eng_max_slots(ve, first_block)) FAIL(e, "window reaches past the prepared batches");
    if (nla_crs_eng_ensure_blocks(e, first_block, first_block + (uint64_t) K)) { if (!e->err[0]) snprintf(e->err, sizeof e->err, "batch preparation failed"); return -1; }
    if ((e->shchain ? window_launch_sh : window_launch)(e, first_block, K, i0, f_best, W, Wf, nW, fwcap)) return -1;
    EVREC(e, e->ev1);
    if (e->idle_fn) e->idle_fn(e->idle_arg);      /* the window is with the device: the driver's upkeep of its ordered set runs beside it */
    CK(e, nla_stream_sync(e->main));              /* status and records were written into pinned host memory by the kernel */
    if (e->shchain) {
        /* record K: whether every rank's share of every slot arrived, and the ranks' agreed stop flags */
        if (e->h_status[K].t != 0) FAIL(e, "a rank's share of a trial point did not arrive within 1.5 s (column-sharded window %u)", e->sh_seq);
        e->stop_out[0] = e->h_status[K].fT != 0.; e->stop_out[1] = e->h_status[K].fM != 0.;
    }
    window_epilogue(e, first_block, K, nW, status, fwcnt, fwrec, fwcap);
    return 0;
}
