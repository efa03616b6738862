/* crs_engine.h — the HIP engine behind the CRS2_LM driver, shared by crs_engine.c (life cycle, batch ring, population init, small ops, ops
 * table), crs_pass.c (the stream work of a pass or a window) and crs_entry.c (API entry points, sessions).  Private; plain C over the C-ABI
 * launchers of include/nlopt_amd.h (no HIP types here).
 * Memory (all HBM, sized for one MI355X; N=1e5, n=4096 is 3.3 GB, N=1e6 33 GB of 288 GB):
 *   X          N x ld fp64 population (the reference's ps matrix without the f column)
 *   block ring 2B stream blocks pre-digested ahead of use, block b at entry b % 2B: words (2n u32), jn/last (i32), pos (n i32); filled one
 *              half (= one batch of B blocks) at a time on the rng stream
 *   slot ring  KCAP slots, block b at slot b & (KCAP-1): TX (partial sum, then the finished trial point), TM (its mutation), fT/fM
 * Streams: `main` runs [upload + commit of the previous pass's accepts] -> advance -> finish -> status D2H -> (host walk) each pass; `rng`
 * runs the MT generator, the GF(2) jumps and the Vitter kernel for the *next* batch of blocks concurrently (VALU-bound work hiding under
 * the HBM-bound gather); an event per batch orders main after rng. */
#ifndef NLA_CRS_ENGINE_H
#define NLA_CRS_ENGINE_H
#include "nla_internal.h"
#include "nla_switches.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define NLA_KC_MAX 16                 /* commits an advance launch can carry (hip/crs_kernels.hip) */
#define KCAP 1024                          /* slot ring (power of two) */
/* the objective id as the kernel launchers take it: a compiled-in objective under nlopt_set_max_objective delivers -f (e->sign) */
#define OBJK(e) (((e)->obj >= 0 && (e)->sign < 0) ? ((e)->obj | NLA_OBJ_NEGATE) : (e)->obj)
#define NLA_KARG_MAX 128                   /* list length that still travels as kernel arguments (hip/crs_kernels.hip NLA_KA_MAX) */
#define ROWPAD 64                          /* spare rows behind X / F: the init all-gather wants equal blocks per rank (world <= 64) */
/* one H2D per pass, packed: [W: nW i64][crow: nc i64][t_in: K i32][cslot: nc i32][ckind: nc i32] */
#define UPLOAD_BYTES (KCAP * (8 + 8 + 4 + 4 + 4))
#define CHAIN_KMAX 256                     /* window slots / worst rows one device-resolved launch handles */
#define CHAIN_FWCAP 48                     /* records per slot (crs_driver.c FWCAP) */
#define NLA_CRS_FORWARD_MIN_N 1       /* device-resolved windows (hip/crs_chain.hip) from this dimension on — every dimension since round 5 (with the resolver
                                        * wavefront the windows beat the conservative passes at n = 64 / 128 / 256 too: profiles/r05_staged_ab.txt); the
                                        * conservative passes remain what host objectives, user kernels, column-sharded multi-rank jobs and "amd_forward" = 0 run on */

typedef struct {
    int64_t index;                 /* batch number (blocks [index*B, (index+1)*B)), -1 = empty */
    void *ev_ready;
    int waited;                    /* main stream already ordered after ev_ready */
} crs_batch;

typedef struct nla_crs_hip_engine nla_crs_hip_engine;
struct nla_crs_hip_engine {
    int n, ld, obj;                /* obj: compiled-in objective id; -1: host callback; -2: user-supplied kernel (user, sign) */
    nla_userobj *user; double sign;
    int32_t *d_list, *h_list;      /* user kernel: the window's slot rows */
    double *h_fTM;                 /* user kernel: fT / fM rings read back (2 x KCAP) */
    int64_t N;
    int B;                         /* blocks per batch; the block ring holds 2B */
    void *main, *rng;
    nla_mtstream *mts;
    double *d_lb, *d_ub, *d_X, *d_F;
    uint32_t *d_initwords;         /* the stream words of one chunk of rows: allocated and freed by init_population, which runs once per engine */
    crs_batch bat[2];
    uint32_t *d_words;             /* 2B x 2n */
    int32_t *d_jn, *d_pos, *d_last;
    double *d_TX, *d_TM, *d_fT, *d_fM;
    char *d_up, *h_up;
    int32_t *d_tout;
    nla_crs_slot_status *d_status, *h_status;
    int32_t h_t[KCAP];             /* picks summed so far, per slot (host-authoritative) */
    int npending;                  /* commits staged on the host, not yet written to X (small lists: done inside the next pass's advance launch) */
    int32_t pend_slot[KCAP], pend_kind[KCAP];
    int64_t pend_row[KCAP];
    void *ev0, *ev1;
    /* the gather kernel is timed with an event pair around it (the roofline figure of bench.py).  A pair costs two barrier packets
     * in front of and behind the kernel: nothing next to a 0.2-3 ms gather, a good part of a 10-20 us pass at small n — there only
     * every TIME_EVERY-th pass is timed; its bytes and its time go into the statistics together (gather_launches counts timed passes) */
    unsigned pass_no; int timed;
    int uncached;                  /* TX / TM / ctrl are uncached memory (the chain kernel may run) */
    int direct_status;             /* the finish kernel writes the status records into pinned host memory itself and rings a word there when the
                                    * last record is visible: the host spins on it instead of sleeping in a stream synchronisation (conservative
                                    * passes with small lists only; NLA_CRS_COPY_STATUS turns it off) */
    uint32_t *h_bell, *d_bellcount, bell_seq;
    void (*idle_fn)(void *); void *idle_arg;   /* the driver's host work beside a pass (ops->set_idle) */
    /* device-resolved windows (hip/crs_chain.hip): control block, the walk's lists when they do not fit the kernel arguments,
     * what every slot took from where (pinned, written by the kernel) */
    void *d_ctrl;
    uint32_t ticket_base;
    uint32_t *h_fwcnt, *h_fwrec;
    double *d_Wf;
    int force_upload;              /* NLA_CRS_UPLOAD: the pass's lists through the H2D copy even when they fit the kernel arguments (A/B switch) */
    FILE *pass_log;                /* NLA_CRS_PASS_LOG=<file>: one line per pass (development aid, see tools/pass_log_summary.py) */
    nlopt_amd_stats *stats;
    nlopt_amd_comm *comm;          /* multi-GPU: NULL = single process */
    /* several GPUs, compiled-in objective: the population is sharded BY COORDINATE (hip/crs_shard.hip) — this rank holds columns
     * [c0, c0 + nc) of every row, c0 = rank * colper, colper = ceil(n / world); ld = the slice's row stride.  Every rank replays the
     * identical chain on identical f values: the candidates of a pass are all-gathered and evaluated by every rank */
    int sharded, world, rank, c0, nc, colper;      /* (single process: c0 = 0, nc = colper = n) */
    double *d_csend, *d_crecv;     /* a pass's candidates: 2 KCAP slices of colper doubles (+ 2 stop flags), world x that */
    int stop_in[2], stop_out[2];   /* the per-process stop conditions: this rank's view into a pass, all ranks' OR out of it */
    double *d_gsend, *d_grecv, *h_g;   /* a whole point from its slices (read_row / read_slot): colper, world x colper */
    const double *h_lb_full, *h_ub_full;   /* the caller's bounds (valid for the engine's life: the run's own arrays) */
    /* column-sharded population with the window resolved ON the device (hip/crs_chain.hip, SH instance; round 6): trial points are whole
     * (rows of ldf doubles) on every rank — a rank's workgroups store their chunk of a slot into every rank's TX through peer-mapped
     * memory — so every rank evaluates and resolves as a single device does and the 128-slot window survives the sharding */
    int shchain, ldf, ncolp;       /* ncolp: columns gathered = nc, even-padded from n = 128 on (the pad column of X is zero) */
    int sh_chunk0, sh_chunks_total;    /* the chunks the ranks' workgroups store a slot in: where this rank's begin, all of them */
    uint32_t sh_seq;
    int sh_grid_cap;               /* ranks sharing one device ("amd_cu_share" = k): each rank's window kernel holds at most its k-th of the chip */
    void *d_shared;                /* ONE peer-mapped block of uncached memory: TX | flags | stop words */
    void *peer_block[8];           /* the other ranks' blocks as mapped here (nla_ipc_open) */
    void *d_table;                 /* what the kernel reads of all this (nla_crs_chain_sh_table) */
    double *d_xbest, *d_lbf, *d_ubf;   /* the whole best row, the whole bounds */
    int64_t xbest_row;             /* the row d_xbest is a copy of (-1: none yet) */
    char err[256];
};

#define FAIL(e, ...) do { snprintf((e)->err, sizeof (e)->err, __VA_ARGS__); return -1; } while (0)
#define CK(e, call) do { int rc_ = (call); if (rc_) FAIL(e, "%.160s failed: %s", #call, nla_dev_error_string(rc_)); } while (0)

/* what an engine is created from.  shard: 0 replicas / single process, 1 column-sharded with conservative passes, 2 column-sharded with
 * device-resolved windows (cu_parts >= 2: the ranks share one device — a test box — and each confines its window kernels to its share of
 * the compute units) */
typedef struct {
    int n; int64_t N; const double *lb, *ub;       /* the bounds are the run's own arrays: they outlive the engine */
    int obj; nla_userobj *user; double sign;       /* compiled-in objective id; -1: host callback; -2: the user's kernel `user` */
    int forward;                                   /* device-resolved windows may run (uncached trial points, the control block) */
    nlopt_amd_comm *comm; int shard, cu_parts; nlopt_amd_stats *stats;
} nla_crs_engine_config;
nla_crs_hip_engine *nla_crs_hip_engine_create(const nla_crs_engine_config *cfg);
void nla_crs_hip_engine_destroy(nla_crs_hip_engine *e, uint64_t words_used);
extern const nla_crs_engine_ops nla_crs_hip_ops;

/* crs_engine.c, for the passes: the batches holding blocks [first, last] usable on the main stream; the ops table's max_slots */
int nla_crs_eng_ensure_blocks(nla_crs_hip_engine *e, uint64_t first, uint64_t last);
int nla_crs_eng_max_slots(void *e, uint64_t first_block);
/* crs_pass.c, for the ops table (advance, chain) and for the ops that read X: the staged commits written to X, stream synchronised */
int nla_crs_eng_advance(void *e, uint64_t first_block, int K, uint64_t fresh_from, int64_t i0, const int64_t *W, int nW, nla_crs_slot_status *status);
int nla_crs_eng_chain(void *e, uint64_t first_block, int K, int64_t i0, double f_best, const int64_t *W, const double *Wf, int nW,
                      nla_crs_slot_status *status, uint32_t *fwcnt, uint32_t *fwrec, int fwcap);
int nla_crs_eng_flush_commits(nla_crs_hip_engine *e);

#endif
