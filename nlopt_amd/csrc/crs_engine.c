/* crs_engine.c — the HIP engine behind the CRS2_LM driver (crs_engine.h): its life cycle, the ring of pre-digested stream blocks,
 * population initialisation, the small ops and the ops table.  What a pass puts on the stream is crs_pass.c. */
#include "crs_engine.h"

#define INIT_CHUNK_WORDS (1ULL << 28)      /* 1 GiB of stream words per init pass */

/* ---- column slices ------------------------------------------------------------------------------------------------------------------- */
/* can n coordinates be dealt over `world` ranks in equal blocks of ceil(n / world) with nobody left empty? */
int nla_crs_can_shard(int n, int world)
{
    if (world < 2) return 0;
    return (int64_t) (world - 1) * ((n + world - 1) / world) < n;
}

/* ... and for the device-resolved windows: equal blocks of whole 128-byte lines (no line of a trial point is written by two ranks),
 * at most 8 ranks (the kernel's peer table) */
static int shchain_colper(int n, int world) { return (((n + world - 1) / world) + 15) & ~15; }
int nla_crs_can_shard_windows(int n, int world)
{
    if (world < 2 || world > 8) return 0;
    return (int64_t) (world - 1) * shchain_colper(n, world) < n;
}

/* rank r holds columns [*c0, *c0 + count) of n dealt in blocks of colper */
static int slice_of(int n, int colper, int r, int *c0) { *c0 = r * colper; return n - *c0 < colper ? n - *c0 : colper; }
/* the columns a window gathers of a slice of nc: even-padded from n = 128 on (the pad column of X is zero) */
static int padded_cols(int n, int nc) { return (n >= 128 && (nc & 1)) ? nc + 1 : nc; }

/* ---- the batch ring ------------------------------------------------------------------------------------------------------------------ */
static uint64_t trial_word0(const nla_crs_hip_engine *e) { return 2ULL * (uint64_t) e->n * (uint64_t) (e->N - 1); }

static int prepare_batch(nla_crs_hip_engine *e, crs_batch *b, int64_t index)
{
    const size_t half = (size_t) (index & 1) * (size_t) e->B;
    const uint64_t w0 = trial_word0(e) + 2ULL * (uint64_t) e->n * (uint64_t) index * (uint64_t) e->B;
    uint32_t *words = e->d_words + half * 2 * (size_t) e->n;
    b->index = index;
    b->waited = 0;
    if (nla_mtstream_fill(e->mts, w0, 2ULL * (uint64_t) e->n * (uint64_t) e->B, words))
        FAIL(e, "MT stream fill failed for batch %lld", (long long) index);
    CK(e, nla_k_crs_vitter(e->n, e->N, words, e->B, e->d_jn + half, e->d_pos + half * (size_t) e->n, e->d_last + half, e->rng));
    CK(e, nla_event_record(b->ev_ready, e->rng));
    return 0;
}

/* make the batches holding blocks [first, last] usable on the main stream (last < first + 2B - B
 * is guaranteed by max_slots: a window never reaches past the batch after first's) */
int nla_crs_eng_ensure_blocks(nla_crs_hip_engine *e, uint64_t first, uint64_t last)
{
    const int64_t i0 = (int64_t) (first / (uint64_t) e->B), i1 = (int64_t) (last / (uint64_t) e->B);
    crs_batch *cur = &e->bat[i0 & 1], *nxt = &e->bat[(i0 + 1) & 1];
    if (i1 > i0 + 1) FAIL(e, "window reaches past the prepared batches");
    /* everything that used the half being overwritten has been consumed: blocks < first are done */
    if (cur->index != i0 && prepare_batch(e, cur, i0)) return -1;
    if (nxt->index != i0 + 1 && prepare_batch(e, nxt, i0 + 1)) return -1;
    if (!cur->waited) { CK(e, nla_stream_wait_event(e->main, cur->ev_ready)); cur->waited = 1; }
    if (i1 > i0 && !nxt->waited) { CK(e, nla_stream_wait_event(e->main, nxt->ev_ready)); nxt->waited = 1; }
    return 0;
}

int nla_crs_eng_max_slots(void *ve, uint64_t first_block)
{
    /* the window and the block after it (mutation words) must lie in first_block's batch or the next */
    nla_crs_hip_engine *e = (nla_crs_hip_engine *) ve;
    const uint64_t B = (uint64_t) e->B;
    uint64_t rem = (first_block / B + 2) * B - 1 - first_block;
    return (int) (rem < KCAP ? rem : KCAP);
}

/* ---- life cycle ---------------------------------------------------------------------------------------------------------------------- */
void nla_crs_hip_engine_destroy(nla_crs_hip_engine *e, uint64_t words_used)
{
    /* trial points: ordinary or uncached memory as create chose (in window mode on a sharded population TX is the front of d_shared) */
    void (*const free_trial)(void *) = e && e->uncached ? nla_dev_free_uncached : nla_dev_free;
    if (!e) return;
    if (e->main) nla_stream_sync(e->main);
    if (e->rng) nla_stream_sync(e->rng);
    if (e->mts) { nla_mtstream_finish(e->mts, words_used); nla_mtstream_destroy(e->mts); }
    if (e->pass_log) fclose(e->pass_log);
    for (int i = 0; i < 2; ++i) nla_event_destroy(e->bat[i].ev_ready);
    nla_dev_free(e->d_words); nla_dev_free(e->d_jn); nla_dev_free(e->d_pos); nla_dev_free(e->d_last);
    nla_dev_free(e->d_lb); nla_dev_free(e->d_ub); nla_dev_free(e->d_X); nla_dev_free(e->d_F);
    nla_dev_free(e->d_initwords);
    for (int r = 0; r < 8; ++r) nla_ipc_close(e->peer_block[r]);
    if ((void *) e->d_TX != e->d_shared) free_trial(e->d_TX);
    free_trial(e->d_TM);
    nla_dev_free_uncached(e->d_shared); nla_dev_free_uncached(e->d_ctrl);
    nla_dev_free(e->d_table); nla_dev_free(e->d_xbest); nla_dev_free(e->d_lbf); nla_dev_free(e->d_ubf);
    nla_dev_free(e->d_fT);   /* d_fM aliases d_fT + KCAP */
    nla_dev_free(e->d_up); nla_dev_free(e->d_tout); nla_dev_free(e->d_status);
    nla_dev_free(e->d_list); nla_host_free(e->h_list); nla_host_free(e->h_fTM);
    nla_dev_free(e->d_Wf); nla_host_free(e->h_fwcnt); nla_host_free(e->h_fwrec);
    nla_host_free(e->h_up); nla_host_free(e->h_status); nla_host_free(e->h_bell); nla_dev_free(e->d_bellcount);
    nla_dev_free(e->d_csend); nla_dev_free(e->d_crecv); nla_dev_free(e->d_gsend); nla_dev_free(e->d_grecv); nla_host_free(e->h_g);
    nla_event_destroy(e->ev0); nla_event_destroy(e->ev1);
    if (e->rng != e->main) nla_stream_destroy(e->rng);
    nla_stream_destroy(e->main);
    free(e);
}

/* create's allocations, `count` elements of T each: a failure clears the flag `ok`, which create looks at once */
static void *alloc_ok(int *ok, void *p) { if (!p) *ok = 0; return p; }
#define DEV(ok, T, count) ((T *) alloc_ok(&(ok), nla_dev_malloc(sizeof(T) * (size_t) (count))))
#define DEV_UC(ok, T, count) ((T *) alloc_ok(&(ok), nla_dev_malloc_uncached(sizeof(T) * (size_t) (count))))
#define PINNED(ok, T, count) ((T *) alloc_ok(&(ok), nla_host_malloc(sizeof(T) * (size_t) (count))))
#define EVENT(ok) alloc_ok(&(ok), nla_event_create())
static size_t shchain_flag_bytes(const nla_crs_hip_engine *e) { return (sizeof(uint32_t) * (size_t) CHAIN_KMAX * (size_t) e->sh_chunks_total + 127) & ~(size_t) 127; }
static int shchain_setup(nla_crs_hip_engine *e, int allocated);

nla_crs_hip_engine *nla_crs_hip_engine_create(const nla_crs_engine_config *cfg)
{
    nla_crs_hip_engine *e;
    const int n = cfg->n, obj = cfg->obj, cu_parts = cfg->cu_parts;
    const int64_t N = cfg->N;
    const char *lg = NLA_DBG_ENV("NLA_CRS_BATCH_LOG2");                /* development switch */
    const int lg2 = lg ? atoi(lg) : 28;
    size_t B, cdoubles;
    int ok = 1;
    if (nla_dev_count() <= 0) return NULL;
    e = (nla_crs_hip_engine *) calloc(1, sizeof *e);
    if (!e) return NULL;
    e->n = n; e->N = N; e->obj = obj; e->user = cfg->user; e->sign = cfg->sign; e->stats = cfg->stats; e->comm = cfg->comm;
    e->h_lb_full = cfg->lb; e->h_ub_full = cfg->ub; e->xbest_row = -1; e->bat[0].index = e->bat[1].index = -1;
    e->world = nlopt_amd_comm_world(e->comm); e->rank = nlopt_amd_comm_rank(e->comm);
    e->sharded = cfg->shard && nla_crs_can_shard(n, e->world) && obj >= 0;
    e->shchain = e->sharded && cfg->shard == 2 && nla_crs_can_shard_windows(n, e->world);
    e->c0 = 0; e->nc = n; e->colper = n;
    /* (measured on this pool, tools/cu_mask_probe.hip: a CU-masked stream still runs on all 256 compute units — so what keeps the kernels of
     * ranks that share a device resident together is the cap on their workgroups: 224 of the chip's 256 one-workgroup-per-CU places dealt
     * over the ranks, the rest left to the generator's kernels) */
    e->sh_grid_cap = cu_parts >= 2 ? (224 / cu_parts >= 4 ? 224 / cu_parts : 4) : 0;
    if (e->sharded) {
        e->colper = e->shchain ? shchain_colper(n, e->world) : (n + e->world - 1) / e->world;
        e->nc = slice_of(n, e->colper, e->rank, &e->c0);
    }
    e->ld = (e->nc + 15) & ~15;
    e->ldf = e->shchain ? ((n + 15) & ~15) : e->ld;
    e->ncolp = padded_cols(n, e->nc);      /* rows start on a 128-byte line (the chain kernel's contract; coalesced row reads everywhere) */
    for (int r = 0, c0r; e->shchain && r < e->world; ++r) {
        if (r == e->rank) e->sh_chunk0 = e->sh_chunks_total;
        e->sh_chunks_total += nla_crs_chain_sh_chunks(n, padded_cols(n, slice_of(n, e->colper, r, &c0r)));
    }
    /* blocks digested per batch (the block ring holds two batches).  The Vitter kernel walks all N rows per block, one lane per
     * block (a serial fp64 chain): a launch takes the same 40-70 ms (N = 1e5) whether it digests 4096 blocks or 32768 — it is
     * the number of lanes, not the time, that grows.  Measured with 4096-block batches at n = 4096 (profiles/r02_v1_kernel_stats.csv):
     * the kernel was running under the gather 40-60 % of the time, on a quarter of the CUs, and the gather's workgroups on those
     * CUs were the last to finish every pass.  With 2^28 words per batch (32768 blocks at n = 4096: 2.1 GB of words + 1 GB of
     * positions in the ring, of 288 GB) it runs a few per cent of the time. */
    B = (size_t) ((1ULL << (lg2 >= 20 && lg2 <= 31 ? lg2 : 28)) / (2ULL * (uint64_t) n));
    B = B > 65536 ? 65536 : (B < 2 * KCAP ? 2 * KCAP : B);
    e->B = (int) B;
    if (NLA_DBG_ENV("NLA_CRS_PASS_LOG")) e->pass_log = fopen(NLA_DBG_ENV("NLA_CRS_PASS_LOG"), "a");
    e->direct_status = !NLA_DBG_ENV("NLA_CRS_COPY_STATUS");
    e->force_upload = NLA_DBG_ENV("NLA_CRS_UPLOAD") != NULL;
    /* "amd_cu_share" = k >= 2: this process's window kernels on every k-th compute unit (ranks that share a device; a single process
     * asks for it to be measured on the same share, tools/shard_probe.py) */
    e->main = cu_parts >= 2 ? nla_stream_create_cu_share(e->rank % cu_parts, cu_parts) : nla_stream_create();
    if (!e->main && cu_parts >= 2) e->main = nla_stream_create();
    /* NLA_ONE_STREAM (A/B switch for debugging stream-ordering problems): the generator work on the main stream too */
    e->rng = NLA_DBG_ENV("NLA_ONE_STREAM") ? e->main : nla_stream_create();      /* (restricting this stream to a subset of the CUs — hipExtStreamCreateWithCUMask, every 4th / 16th CU — was measured:
                                        *  43.0 -> 43.1 k evals/s; what the digest kernels cost the gather is memory traffic, not CUs) */
    if (!e->main || !e->rng || !(e->mts = nla_mtstream_create(e->rng))) goto fail;
    e->d_lb = DEV(ok, double, e->ld); e->d_ub = DEV(ok, double, e->ld);
    e->d_X = DEV(ok, double, (size_t) e->ld * (size_t) (N + ROWPAD)); e->d_F = DEV(ok, double, N + ROWPAD);
    e->d_words = DEV(ok, uint32_t, 2 * (size_t) n * 2 * B);
    e->d_jn = DEV(ok, int32_t, 2 * B); e->d_last = DEV(ok, int32_t, 2 * B); e->d_pos = DEV(ok, int32_t, 2 * B * (size_t) n);
    e->bat[0].ev_ready = EVENT(ok); e->bat[1].ev_ready = EVENT(ok);
    /* trial points and the chain kernel's control block: uncached memory where the workgroups of one launch read each other's
     * (device-resolved windows); ordinary memory for the conservative passes, whose kernels meet only at launch boundaries */
    e->uncached = ((e->sharded ? e->shchain : cfg->forward) && obj >= 0) || NLA_DBG_ENV("NLA_UC_ALWAYS") != NULL;       /* (NLA_UC_ALWAYS: round 2's allocation pattern, A/B) */
    if (e->shchain) {
        /* whole trial points; TX, the chunk flags and the stop words in one block the other ranks map */
        const size_t txb = sizeof(double) * (size_t) e->ldf * KCAP, flb = shchain_flag_bytes(e);
        e->d_shared = DEV_UC(ok, char, txb + flb + nla_crs_chain_sh_stop_bytes());
        e->d_TX = (double *) e->d_shared;
        if (e->d_shared && nla_memset((char *) e->d_shared + txb, 0, flb + nla_crs_chain_sh_stop_bytes(), e->main)) ok = 0;
        e->d_TM = DEV_UC(ok, double, (size_t) e->ldf * KCAP);
        e->d_table = DEV(ok, char, nla_crs_chain_sh_table_bytes());
        e->d_xbest = DEV(ok, double, e->ldf); e->d_lbf = DEV(ok, double, e->ldf); e->d_ubf = DEV(ok, double, e->ldf);
    } else if (e->uncached) { e->d_TX = DEV_UC(ok, double, (size_t) e->ld * KCAP); e->d_TM = DEV_UC(ok, double, (size_t) e->ld * KCAP); }
    else { e->d_TX = DEV(ok, double, (size_t) e->ld * KCAP); e->d_TM = DEV(ok, double, (size_t) e->ld * KCAP); }
    e->d_fT = DEV(ok, double, 2 * KCAP); e->d_fM = e->d_fT ? e->d_fT + KCAP : NULL;
    e->d_up = DEV(ok, char, UPLOAD_BYTES); e->d_tout = DEV(ok, int32_t, KCAP); e->d_status = DEV(ok, nla_crs_slot_status, KCAP + 1);
    e->h_up = PINNED(ok, char, UPLOAD_BYTES); e->h_status = PINNED(ok, nla_crs_slot_status, KCAP + 1);
    e->ev0 = EVENT(ok); e->ev1 = EVENT(ok);
    if (obj == -2) { e->d_list = DEV(ok, int32_t, KCAP); e->h_list = PINNED(ok, int32_t, KCAP); e->h_fTM = PINNED(ok, double, 2 * KCAP); }
    if (e->uncached && obj >= 0) {
        e->d_ctrl = DEV_UC(ok, char, nla_crs_chain_ctrl_bytes(CHAIN_KMAX, CHAIN_KMAX)); e->d_Wf = DEV(ok, double, CHAIN_KMAX);
        e->h_fwcnt = PINNED(ok, uint32_t, CHAIN_KMAX); e->h_fwrec = PINNED(ok, uint32_t, CHAIN_KMAX * CHAIN_FWCAP);
    }
    e->h_bell = PINNED(ok, uint32_t, 16);       /* (explicitly coherent pinned memory measured equal within noise, profiles/r04_crs_doorbell_ab.txt: the
                                             * finish kernel's system-scope fence is what makes the records visible before the bell) */
    e->d_bellcount = DEV(ok, uint32_t, 16);
    /* a sharded run's exchange buffers (the candidates' all-gather buffers serve the conservative passes only: a window-mode run
     * exchanges nothing by collective) */
    cdoubles = (e->shchain ? 1 : 2 * KCAP) * (size_t) e->colper + 2;
    if (e->sharded) {
        e->d_csend = DEV(ok, double, cdoubles); e->d_crecv = DEV(ok, double, cdoubles * (size_t) e->world);
        e->d_gsend = DEV(ok, double, e->colper); e->d_grecv = DEV(ok, double, (size_t) e->colper * (size_t) e->world);
        e->h_g = PINNED(ok, double, (size_t) e->colper * (size_t) e->world);
    }
    if (!ok) {
        /* (a window-mode rank still joins the handle exchange below, saying it failed: the others must not wait for it there) */
        if (e->shchain) shchain_setup(e, 0);
        goto fail;
    }
    if (e->sharded) {
        /* the communicator's staging for the largest exchange of the run — a pass's candidates, or a rank's share of the initial
         * values — now, while a failure can still be agreed on (the set-up's "ready" exchange), not inside a collective */
        const size_t ini = (size_t) ((e->N - 1 + e->world - 1) / e->world);
        if (nla_comm_reserve(e->comm, sizeof(double) * (cdoubles > ini ? cdoubles : ini))) goto fail;
        if (nla_memset(e->d_gsend, 0, sizeof(double) * (size_t) e->colper, e->main) || nla_memset(e->d_csend, 0, sizeof(double) * cdoubles, e->main)) goto fail;
    }
    *e->h_bell = 0;
    if (nla_memset(e->d_bellcount, 0, 64, e->main)) goto fail;
    /* the slice's bounds (the whole vectors in a single-process run); pad entries are zero */
    if ((e->d_ctrl && nla_memset(e->d_ctrl, 0, nla_crs_chain_ctrl_bytes(CHAIN_KMAX, CHAIN_KMAX), e->main)) ||
        nla_memset(e->d_lb, 0, sizeof(double) * (size_t) e->ld, e->main) || nla_memset(e->d_ub, 0, sizeof(double) * (size_t) e->ld, e->main) ||
        nla_memcpy_h2d(e->d_lb, cfg->lb + e->c0, sizeof(double) * (size_t) e->nc, e->main) ||
        nla_memcpy_h2d(e->d_ub, cfg->ub + e->c0, sizeof(double) * (size_t) e->nc, e->main) || nla_stream_sync(e->main)) goto fail;
    if (e->shchain && shchain_setup(e, 1)) goto fail;
    return e;
fail:
    nla_crs_hip_engine_destroy(e, 0);
    return NULL;
}

/* window-mode set-up: every rank exports its peer-mapped block, the handles are all-gathered (host data: 96 bytes per rank), every rank
 * maps the others' blocks and writes its table.  A rank whose allocations failed (allocated = 0) takes part with an invalid handle, so
 * that nobody waits for it; every rank then fails the set-up (the caller falls back to the conservative passes, on all ranks alike). */
static int shchain_setup(nla_crs_hip_engine *e, int allocated)
{
    unsigned char mine[NLA_IPC_BYTES], all[8 * NLA_IPC_BYTES];
    void *ptx[8], *pfl[8], *pst[8];
    char *img;
    const size_t txb = sizeof(double) * (size_t) e->ldf * KCAP, flb = shchain_flag_bytes(e);
    int ok = allocated, bad = 0;
    memset(mine, 0, sizeof mine);
    if (ok && (nla_stream_sync(e->main) || nla_ipc_export(e->d_shared, mine))) { ok = 0; memset(mine, 0, sizeof mine); }
    if (nla_comm_allgather_host(e->comm, mine, all, NLA_IPC_BYTES, e->main)) FAIL(e, "exchange of the window buffers' handles failed: %s", nlopt_amd_comm_error(e->comm));
    for (int r = 0; r < e->world; ++r) {
        int zero = 1;
        for (int i = 0; i < NLA_IPC_BYTES; ++i) if (all[r * NLA_IPC_BYTES + i]) { zero = 0; break; }
        if (zero) bad = 1;
    }
    if (!ok || bad) FAIL(e, "%s", ok ? "another rank could not set up its window buffers" : "window buffers: allocation or export failed");
    for (int r = 0; r < e->world; ++r) {
        char *base;
        if (r == e->rank) base = (char *) e->d_shared;
        else {
            e->peer_block[r] = nla_ipc_open(all + r * NLA_IPC_BYTES);
            if (!e->peer_block[r]) { bad = 1; base = (char *) e->d_shared; }      /* (agreed below) */
            else base = (char *) e->peer_block[r];
        }
        ptx[r] = base; pfl[r] = base + txb; pst[r] = base + txb + flb;
    }
    /* all ranks mapped all blocks, or none goes on */
    if (!nla_comm_agree_ready(e->comm, !bad) || bad) FAIL(e, "%s", bad ? "mapping a peer's window buffers failed (hipIpcOpenMemHandle)" : "another rank could not map the window buffers");
    img = (char *) malloc(nla_crs_chain_sh_table_bytes());
    if (!img) FAIL(e, "out of memory");
    if (nla_crs_chain_sh_table(img, e->world, e->rank, e->c0, e->ldf, e->sh_chunks_total, e->sh_chunk0, ptx, pfl, pst, e->d_xbest, e->d_lbf, e->d_ubf) ||
        nla_memcpy_h2d(e->d_table, img, nla_crs_chain_sh_table_bytes(), e->main) ||
        nla_memset(e->d_lbf, 0, sizeof(double) * (size_t) e->ldf, e->main) || nla_memset(e->d_ubf, 0, sizeof(double) * (size_t) e->ldf, e->main) ||
        nla_memset(e->d_xbest, 0, sizeof(double) * (size_t) e->ldf, e->main) ||
        nla_memcpy_h2d(e->d_lbf, e->h_lb_full, sizeof(double) * (size_t) e->n, e->main) ||
        nla_memcpy_h2d(e->d_ubf, e->h_ub_full, sizeof(double) * (size_t) e->n, e->main) || nla_stream_sync(e->main)) { free(img); FAIL(e, "window table upload failed"); }
    free(img);
    return 0;
}

/* ---- population initialisation --------------------------------------------------------------------------------------------------------- */
/* development aid (NLA_CRS_DEBUG_DIR=<dir>): what the init kernels saw and made — the stream words, the rows and their f — of the
 * LAST run, as <dir>/init_last.bin: header {n, ld, N, nwords, origin} (5 x i64), words (u32), X (N x ld f64), F (N f64).  A harness
 * that finds a run diverging from the oracle keeps the file and can tell wrong words from wrong rows from wrong values. */
static void dump_init(nla_crs_hip_engine *e, size_t nwords)
{
    char path[512];
    FILE *fp;
    const size_t nx = (size_t) e->N * (size_t) e->ld;
    int64_t hdr[5] = { e->n, e->ld, e->N, (int64_t) nwords, (int64_t) nla_mtstream_origin(e->mts) };
    uint32_t *w = (uint32_t *) malloc(sizeof(uint32_t) * (nwords ? nwords : 1));
    double *x = (double *) malloc(sizeof(double) * (nx + (size_t) e->N));
    if (w && x && !nla_memcpy_d2h(w, e->d_initwords, sizeof(uint32_t) * nwords, e->main) &&
        !nla_memcpy_d2h(x, e->d_X, sizeof(double) * nx, e->main) && !nla_memcpy_d2h(x + nx, e->d_F, sizeof(double) * (size_t) e->N, e->main) &&
        !nla_stream_sync(e->main)) {
        snprintf(path, sizeof path, "%s/init_last.bin", NLA_DBG_ENV("NLA_CRS_DEBUG_DIR"));
        if ((fp = fopen(path, "wb"))) {
            fwrite(hdr, sizeof hdr, 1, fp); fwrite(w, sizeof(uint32_t), nwords, fp); fwrite(x, sizeof(double), nx + (size_t) e->N, fp);
            fclose(fp);
        }
    }
    free(w); free(x);
}

/* the rows of the population dealt over the ranks in equal blocks: rank r's rows are [first, last) = [1 + r per, 1 + (r+1) per) below N */
typedef struct { int64_t per, first, last; } init_rows;
static init_rows init_rows_of_rank(const nla_crs_hip_engine *e)
{
    const int64_t per = (e->N - 1 + e->world - 1) / e->world, first = 1 + per * e->rank;
    return (init_rows) { per, first, first + per < e->N ? first + per : e->N };
}

/* rows whose stream words (2n each) fit one chunk of the words buffer: at least one, at most `most` */
static int64_t init_rows_per_chunk(const nla_crs_hip_engine *e, int64_t most)
{ const int64_t rows = (int64_t) (INIT_CHUNK_WORDS / (2ULL * (uint64_t) e->n)); return rows < 1 ? 1 : (rows > most ? most : rows); }

/* rows [from, to) in chunks: the generator fills the chunk's words on `rng`, the init kernels consume them on `main`, an event hands
 * over both ways.  One device or replicas: the kernels make the rows and their values.  A column-sharded population (mine != NULL): this
 * rank's columns of the rows, and the values of those of ITS rows [mine->first, mine->last) that lie in the chunk, straight from the
 * words with the whole bounds d_lbf / d_ubf.  NULL, or what failed */
static const char *init_chunks(nla_crs_hip_engine *e, int64_t from, int64_t to, int64_t rows_per_chunk, void *ev,
                               const init_rows *mine, const double *d_lbf, const double *d_ubf)
{
    const int n = e->n;
    const uint64_t wpr = 2ULL * (uint64_t) n;            /* words per row */
    for (int64_t r0 = from; r0 < to; r0 += rows_per_chunk) {
        const int64_t nr = to - r0 < rows_per_chunk ? to - r0 : rows_per_chunk;
        int failed;
        /* the words buffer is reused: the generator must not overwrite it before the previous
         * chunk's init kernel has consumed it */
        if (r0 > from && (nla_event_record(ev, e->main) || nla_stream_wait_event(e->rng, ev))) return "event failed";
        if (nla_mtstream_fill(e->mts, wpr * (uint64_t) (r0 - 1), wpr * (uint64_t) nr, e->d_initwords)) return "MT stream fill failed (init)";
        if (nla_event_record(ev, e->rng) || nla_stream_wait_event(e->main, ev)) return "event failed";
        if (mine) {
            const int64_t lo = mine->first > r0 ? mine->first : r0, hi = mine->last < r0 + nr ? mine->last : r0 + nr;
            failed = nla_k_crs_sh_init_rows(n, e->c0, e->nc, e->ld, e->d_lb, e->d_ub, e->d_initwords, r0, nr, e->d_X, e->main) ||
                     (hi > lo && nla_k_crs_init_rows(OBJK(e), n, n, d_lbf, d_ubf, e->d_initwords + (size_t) (lo - r0) * (size_t) wpr, lo, hi - lo, NULL, e->d_F, e->main));
        } else
            failed = nla_k_crs_init_rows(e->obj >= 0 ? OBJK(e) : -1, n, e->ld, e->d_lb, e->d_ub, e->d_initwords, r0, nr, e->d_X, e->d_F, e->main) ||
                     (e->obj == -2 && nla_userobj_eval_rows(e->user, n, e->ld, nr, e->d_X + (size_t) r0 * (size_t) e->ld, e->d_F + r0, NULL, e->sign, e->main));
        if (failed) return "init kernel launch failed";
    }
    return NULL;
}

/* the all-gather between the two events into the statistics */
static void init_allgather_stats(nla_crs_hip_engine *e, void *ev0, void *ev1, uint64_t bytes)
{
    if (!ev0 || !ev1 || !e->stats) return;
    e->stats->t_allgather_ms += (double) nla_event_elapsed_ms(ev0, ev1);
    e->stats->allgather_bytes += bytes;
}

/* crs_init's row loop on a column-sharded population.  Every rank draws ITS columns of every row from the same stream words (row
 * i >= 1 owns words [2n(i-1), 2n i), coordinate j the pair at 2j).  The objective needs whole rows: the ROWS are dealt over the
 * ranks in blocks for that — rank r evaluates rows [1 + r per, 1 + (r+1) per) straight from the words (crs_init_rows_kernel without
 * the store: the same reduction as a single-GPU run, bit for bit) — and the f values are all-gathered in place (8 bytes per row).
 * Nothing of the population itself travels. */
static int init_population_sharded(nla_crs_hip_engine *e, const double *x0, double *F)
{
    const int n = e->n;
    const init_rows rows = init_rows_of_rank(e);                       /* rows per rank (evaluation) */
    const int64_t rows_per_chunk = init_rows_per_chunk(e, e->N - 1);
    void *ev = nla_event_create(), *ev_ag0 = nla_event_create(), *ev_ag1 = nla_event_create();
    double *h_row = (double *) calloc((size_t) (e->ld > n ? e->ld : n), sizeof(double));
    double *d_lbf = NULL, *d_ubf = NULL, *d_x0 = NULL;                 /* whole-row bounds and starting guess (evaluation only) */
    const char *what;
    int rc = -1, stage_ok = 0;
    if (e->world > ROWPAD) { snprintf(e->err, sizeof e->err, "more than %d ranks are not supported", ROWPAD); goto out; }   /* (the same on every rank) */
    e->d_initwords = (uint32_t *) nla_dev_malloc(sizeof(uint32_t) * (size_t) rows_per_chunk * 2 * (size_t) n);
    d_lbf = (double *) nla_dev_malloc(sizeof(double) * (size_t) n);
    d_ubf = (double *) nla_dev_malloc(sizeof(double) * (size_t) n);
    d_x0 = (double *) nla_dev_malloc(sizeof(double) * (size_t) n);
    {   /* all ranks go into the all-gather below, or none (comm.c, nla_comm_agree_ready) */
        const int mine = ev && ev_ag0 && ev_ag1 && h_row && e->d_initwords && d_lbf && d_ubf && d_x0;
        if (!nla_comm_agree_ready(e->comm, mine) || !mine) {
            snprintf(e->err, sizeof e->err, "%s", mine ? "another rank ran out of memory (init)" : "out of memory (init)");
            goto out;
        }
    }
    if (nla_memcpy_h2d(d_lbf, e->h_lb_full, sizeof(double) * (size_t) n, e->main) || nla_memcpy_h2d(d_ubf, e->h_ub_full, sizeof(double) * (size_t) n, e->main) ||
        nla_memcpy_h2d(d_x0, x0, sizeof(double) * (size_t) n, e->main)) { snprintf(e->err, sizeof e->err, "H2D (init) failed"); goto agree2; }
    /* row 0 = the caller's starting guess (crs.c:204): its slice (pad zero), and its value from the whole point */
    memcpy(h_row, x0 + e->c0, sizeof(double) * (size_t) e->nc);
    if (nla_memcpy_h2d(e->d_X, h_row, sizeof(double) * (size_t) e->ld, e->main) ||
        nla_k_eval(OBJK(e), n, n, d_x0, 1, e->d_F, e->main) || nla_stream_sync(e->main)) { snprintf(e->err, sizeof e->err, "row 0 failed"); goto agree2; }
    what = init_chunks(e, 1, e->N, rows_per_chunk, ev, &rows, d_lbf, d_ubf);
    if (what) { snprintf(e->err, sizeof e->err, "%s", what); goto agree2; }
    stage_ok = 1;
agree2:
    /* every rank arrives here, whatever happened to it since the first agreement (H2D copies, fills, launches): all of them go
     * into the all-gather of the values, or none — a rank that failed alone would leave the others waiting in it */
    if (!nla_comm_agree_ready(e->comm, stage_ok) || !stage_ok) {
        if (stage_ok) snprintf(e->err, sizeof e->err, "another rank failed while it initialised its slice of the population");
        goto out;
    }
    nla_event_record(ev_ag0, e->main);
    if (nla_comm_allgather_dev(e->comm, e->d_F + rows.first, e->d_F + 1, sizeof(double) * (size_t) rows.per, e->main)) {
        snprintf(e->err, sizeof e->err, "all-gather of the initial values failed: %s", nlopt_amd_comm_error(e->comm)); nla_comm_abort(e->comm); goto out;
    }
    nla_event_record(ev_ag1, e->main);
    {   /* ... and all of them leave the initialisation together */
        const int mine = !(nla_memcpy_d2h(F, e->d_F, sizeof(double) * (size_t) e->N, e->main) || nla_stream_sync(e->main));
        if (!nla_comm_agree_ready(e->comm, mine) || !mine) {
            snprintf(e->err, sizeof e->err, "%s", mine ? "another rank could not read back the initial values" : "D2H F failed");
            goto out;
        }
    }
    init_allgather_stats(e, ev_ag0, ev_ag1, (uint64_t) e->world * (uint64_t) rows.per * sizeof(double));
    rc = 0;
out:
    nla_event_destroy(ev); nla_event_destroy(ev_ag0); nla_event_destroy(ev_ag1);
    free(h_row);
    nla_dev_free(d_lbf); nla_dev_free(d_ubf); nla_dev_free(d_x0);
    nla_dev_free(e->d_initwords); e->d_initwords = NULL;
    if (rc) return -1;
    return nla_crs_eng_ensure_blocks(e, 0, 0);
}

/* crs_init's row loop (crs.c:211-226).  Row i >= 1 owns stream words [2n(i-1), 2n i), so any block of
 * rows can be produced independently: with a communicator, rank r generates and evaluates rows
 * [1 + r*per, 1 + (r+1)*per) and the rows and their f are ALL-GATHERED in place ("CRS
 * init"); every rank then holds the whole population and runs the identical trial chain. */
static int op_init_population(void *ve, const double *x0, double *F)
{
    nla_crs_hip_engine *e = (nla_crs_hip_engine *) ve;
    const int n = e->n, world = e->world;
    const init_rows rows = init_rows_of_rank(e);                       /* this rank's rows */
    const int64_t rows_per_chunk = init_rows_per_chunk(e, rows.per);
    void *ev, *ev_ag0 = NULL, *ev_ag1 = NULL;
    const char *what = NULL;          /* non-NULL from the first failure on: its message is in e->err */
    int rc;
    if (e->sharded) return init_population_sharded(e, x0, F);
    if (world > ROWPAD) FAIL(e, "more than %d ranks are not supported", ROWPAD);          /* (the same on every rank) */
    ev = nla_event_create();
    if (rows.last > rows.first) e->d_initwords = (uint32_t *) nla_dev_malloc(sizeof(uint32_t) * (size_t) rows_per_chunk * 2 * (size_t) n);
    {   /* several ranks: all of them go into the all-gathers below, or none (comm.c, nla_comm_agree_ready) */
        const int mine = ev && (rows.last <= rows.first || e->d_initwords);
        if (!nla_comm_agree_ready(e->comm, mine) || !mine) {
            nla_event_destroy(ev);
            FAIL(e, "%s", mine ? "another rank ran out of memory (init)" : (ev ? "out of device memory (init words)" : "event create failed"));
        }
    }
    /* row 0 = the caller's starting guess (crs.c:204) */
    if (nla_memcpy_h2d(e->d_X, x0, sizeof(double) * (size_t) n, e->main)) what = "H2D x0 failed";
    else if (e->obj >= 0 && nla_k_eval(OBJK(e), n, e->ld, e->d_X, 1, e->d_F, e->main)) what = "eval launch failed";
    else if (e->obj == -2 && nla_userobj_eval_rows(e->user, n, e->ld, 1, e->d_X, e->d_F, NULL, e->sign, e->main)) what = "user objective launch failed";
    else what = init_chunks(e, rows.first, rows.last, rows_per_chunk, ev, NULL, NULL, NULL);
    if (what) snprintf(e->err, sizeof e->err, "%s", what);
    if (!what && world > 1) {
        ev_ag0 = nla_event_create(); ev_ag1 = nla_event_create();
        if (ev_ag0) nla_event_record(ev_ag0, e->main);
        if (nla_comm_allgather_dev(e->comm, e->d_X + (size_t) rows.first * (size_t) e->ld, e->d_X + (size_t) e->ld,
                                   sizeof(double) * (size_t) rows.per * (size_t) e->ld, e->main) ||
            (e->obj != -1 && nla_comm_allgather_dev(e->comm, e->d_F + rows.first, e->d_F + 1, sizeof(double) * (size_t) rows.per, e->main))) {
            what = "all-gather"; snprintf(e->err, sizeof e->err, "all-gather of the initial population failed: %s", nlopt_amd_comm_error(e->comm));
        } else if (ev_ag1) nla_event_record(ev_ag1, e->main);
    }
    if (!what && e->obj != -1 && nla_memcpy_d2h(F, e->d_F, sizeof(double) * (size_t) e->N, e->main)) { what = "D2H"; snprintf(e->err, sizeof e->err, "D2H F failed"); }
    if (!what && (rc = nla_stream_sync(e->main)) != 0) { what = "sync"; snprintf(e->err, sizeof e->err, "init sync failed: %s", nla_dev_error_string(rc)); }
    if (!what) init_allgather_stats(e, ev_ag0, ev_ag1, (uint64_t) world * (uint64_t) rows.per * (sizeof(double) * (uint64_t) e->ld + (e->obj != -1 ? sizeof(double) : 0)));
    nla_event_destroy(ev); nla_event_destroy(ev_ag0); nla_event_destroy(ev_ag1);
    if (!what && NLA_DBG_ENV("NLA_CRS_DEBUG_DIR") && world == 1 && rows_per_chunk >= rows.per) dump_init(e, (size_t) (2ULL * (uint64_t) n * (uint64_t) (e->N - 1)));
    nla_dev_free(e->d_initwords); e->d_initwords = NULL;
    /* start digesting the first batch of trial blocks while the host builds its ordered set */
    return what ? -1 : nla_crs_eng_ensure_blocks(e, 0, 0);
}

/* ---- the small ops ------------------------------------------------------------------------------------------------------------------- */
/* staged; written to X by the next pass's single upload (or by a flush when something reads X) */
static int op_commit(void *ve, int ncommit, const uint64_t *block, const int32_t *kind, const int64_t *row)
{
    nla_crs_hip_engine *e = (nla_crs_hip_engine *) ve;
    if (ncommit <= 0) return 0;
    if (e->npending && nla_crs_eng_flush_commits(e)) return -1;
    if (ncommit > KCAP) FAIL(e, "too many commits");
    for (int c = 0; c < ncommit; ++c) { e->pend_slot[c] = (int32_t) (block[c] & (KCAP - 1)); e->pend_kind[c] = kind[c]; e->pend_row[c] = row[c]; }
    e->npending = ncommit;
    return 0;
}

/* (a rank that fails in gather_point cannot tell the others in band — they are waiting in this very exchange: nla_comm_abort) */
#define GP(e, call, what) do { int rc_ = (call); if (rc_) { snprintf((e)->err, sizeof (e)->err, "%s failed: %s", what, nla_dev_error_string(rc_)); nla_comm_abort((e)->comm); return -1; } } while (0)

/* a whole point from its column slices: every rank contributes the nc coordinates it holds of the row at `src`, all-gathered */
static int gather_point(nla_crs_hip_engine *e, const double *src, double *x)
{
    GP(e, nla_memcpy_d2d(e->d_gsend, src, sizeof(double) * (size_t) e->nc, e->main), "gather_point: D2D");
    if (nla_comm_allgather_dev(e->comm, e->d_gsend, e->d_grecv, sizeof(double) * (size_t) e->colper, e->main)) {
        nla_comm_abort(e->comm);
        FAIL(e, "all-gather of a point's slices failed: %s", nlopt_amd_comm_error(e->comm));
    }
    GP(e, nla_memcpy_d2h(e->h_g, e->d_grecv, sizeof(double) * (size_t) e->colper * (size_t) e->world, e->main), "gather_point: D2H");
    GP(e, nla_stream_sync(e->main), "gather_point: synchronisation");
    for (int r = 0; r < e->world; ++r) {
        int c0;
        const int cnt = slice_of(e->n, e->colper, r, &c0);
        memcpy(x + c0, e->h_g + (size_t) r * (size_t) e->colper, sizeof(double) * (size_t) cnt);
    }
    return 0;
}

/* a point this rank holds whole */
static int read_point(nla_crs_hip_engine *e, const double *src, double *x)
{
    CK(e, nla_memcpy_d2h(x, src, sizeof(double) * (size_t) e->n, e->main));
    CK(e, nla_stream_sync(e->main));
    return 0;
}

static int op_read_slot(void *ve, uint64_t block, int kind, double *x)
{
    nla_crs_hip_engine *e = (nla_crs_hip_engine *) ve;
    const double *slots = kind == 1 ? e->d_TX : e->d_TM, *src = slots + (size_t) (block & (KCAP - 1)) * (size_t) e->ld;
    if (e->shchain) return read_point(e, slots + (size_t) (block & (KCAP - 1)) * (size_t) e->ldf, x);      /* whole points on every rank: no exchange */
    if (nla_crs_eng_flush_commits(e)) return -1;
    return e->sharded ? gather_point(e, src, x) : read_point(e, src, x);
}

static int op_read_row(void *ve, int64_t row, double *x)
{
    nla_crs_hip_engine *e = (nla_crs_hip_engine *) ve;
    const double *src = e->d_X + (size_t) row * (size_t) e->ld;
    if (nla_crs_eng_flush_commits(e)) return -1;
    return e->sharded ? gather_point(e, src, x) : read_point(e, src, x);
}

static int op_mutate_slot(void *ve, uint64_t block, int64_t i0)
{
    nla_crs_hip_engine *e = (nla_crs_hip_engine *) ve;
    const uint32_t ring = 2u * (uint32_t) e->B;
    if (nla_crs_eng_ensure_blocks(e, block, block + 1) || nla_crs_eng_flush_commits(e)) return -1;
    CK(e, nla_k_crs_mutate(e->n, e->d_X + (size_t) i0 * (size_t) e->ld, e->d_TX + (size_t) (block & (KCAP - 1)) * (size_t) e->ld,
                           e->d_words + (size_t) ((block + 1) % ring) * 2 * (size_t) e->n, e->d_lb, e->d_ub, e->main));
    return 0;
}

static const char *op_last_error(void *ve) { return ((nla_crs_hip_engine *) ve)->err; }
static void op_stop_flags_in(void *ve, int forced, int timed) { nla_crs_hip_engine *e = (nla_crs_hip_engine *) ve; e->stop_in[0] = forced != 0; e->stop_in[1] = timed != 0; }
static void op_stop_flags_out(void *ve, int *forced, int *timed) { nla_crs_hip_engine *e = (nla_crs_hip_engine *) ve; *forced = e->stop_out[0]; *timed = e->stop_out[1]; }
static void op_set_idle(void *ve, void (*fn)(void *), void *arg) { nla_crs_hip_engine *e = (nla_crs_hip_engine *) ve; e->idle_fn = fn; e->idle_arg = arg; }

static int op_reset_slot(void *ve, uint64_t block) { ((nla_crs_hip_engine *) ve)->h_t[block & (KCAP - 1)] = 0; return 0; }

const nla_crs_engine_ops nla_crs_hip_ops = {
    op_init_population, nla_crs_eng_max_slots, nla_crs_eng_advance, nla_crs_eng_chain, op_reset_slot, op_commit, op_read_slot, op_read_row, op_mutate_slot, op_last_error,
    op_stop_flags_in, op_stop_flags_out, op_set_idle
};
