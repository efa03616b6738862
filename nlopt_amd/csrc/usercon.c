/* usercon.c — user-supplied device constraints (include/nlopt_amd.h part 1, include/nlopt_amd_device.h): the sibling of userobj.c.
 *
 * The reference's constraints are host callbacks (src/api/nlopt.h:64-66).  A bound block is a loaded code object and its
 * <name>_coneval kernel; it enters the nlopt_opt as ONE ordinary m-dimensional constraint whose mf is the adapter below and whose
 * f_data is the block:
 *   NLOPT_GN_ISRES          nla_usercon_eval_rows   one launch per block and generation, one wavefront per candidate (isres_driver.c)
 *   anything else           the adapter: the host twin if the user gave one, else a single point through the same kernel
 * Ownership: EVERY constraint entry with mf == adapter owns one reference to its block.  api_options.c retains it wherever such an entry
 * comes to be — the adders (so also AUGLAG's hand-over of (mf, f_data) to its subsidiary optimiser) and nlopt_copy — releases it in
 * nlopt_remove_*_constraints / nlopt_destroy, and SKIPS such entries in the loops that hand constraint data to the caller's
 * nlopt_set_munge / nlopt_munge_data hooks: those would take the block pointer for the caller's own data. */
#include "nla_internal.h"
#include <math.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

struct nla_usercon {
    int refs;
    unsigned m;
    void *module, *fn;
    int abi;                               /* 1: <name>_coneval; 2: <name>_coneval_d, which also takes the block's data */
    void *d_data; size_t data_bytes;       /* ABI 2: the caller's bytes in device memory, owned by the block like its kernel */
    nlopt_mfunc twin; void *twin_data;
    /* single-point evaluation through the kernel (adapter): one scratch set per block, shared by nlopt_copy copies: serialised on `lock` */
    pthread_mutex_t lock;
    void *st;
    double *d_x, *d_c, *h_buf;             /* h_buf pinned: x | c */
    int cap;
};

nla_usercon *nla_usercon_retain(nla_usercon *u) { if (u) __atomic_add_fetch(&u->refs, 1, __ATOMIC_RELAXED); return u; }
void nla_usercon_release(nla_usercon *u)
{
    if (!u || __atomic_sub_fetch(&u->refs, 1, __ATOMIC_ACQ_REL) > 0) return;
    if (u->st) nla_stream_sync(u->st);
    nla_dev_free(u->d_x); nla_dev_free(u->d_c); nla_dev_free(u->d_data); nla_host_free(u->h_buf);
    if (u->st) nla_stream_destroy(u->st);
    nla_module_unload(u->module);
    pthread_mutex_destroy(&u->lock);
    free(u);
}

/* C[row * ldc + j] = value j of the block at row `row` of X, row < count, j < m */
int nla_usercon_eval_rows(nla_usercon *u, int n, int ld, int64_t count, const double *X, int ldc, double *C, void *stream)
{
    /* <name>_coneval(int n, int ld, long count, const double *X, int m, int ldc, double *C)
     * <name>_coneval_d(the same, const void *data, size_t data_bytes) */
    int32_t an = n, ald = ld, am = (int32_t) u->m, aldc = ldc;
    int64_t acount = count;
    const void *adata = u->d_data;
    size_t abytes = u->data_bytes;
    void *params[9];
    if (count <= 0) return 0;
    params[0] = &an; params[1] = &ald; params[2] = &acount; params[3] = &X; params[4] = &am; params[5] = &aldc; params[6] = &C;
    params[7] = &adata; params[8] = &abytes;       /* (ABI 1 takes the first seven) */
    return nla_module_launch(u->fn, (unsigned) ((count + 3) / 4), 256, params, stream);
}

/* the block as an ordinary nlopt_mfunc: the host twin if the user gave one, else one point through the kernel (values only) */
static void adapter(unsigned m, double *result, unsigned n, const double *x, double *grad, void *data)
{
    nla_usercon *u = (nla_usercon *) data;
    const int ld = (int) ((n + 1) & ~1u);
    unsigned j;
    int ok = 0;
    if (u->twin) { u->twin(m, result, n, x, grad, u->twin_data); return; }
    pthread_mutex_lock(&u->lock);
    if ((int) n > u->cap) {
        nla_dev_free(u->d_x); nla_host_free(u->h_buf);
        u->d_x = (double *) nla_dev_malloc(sizeof(double) * (size_t) ld);
        u->h_buf = (double *) nla_host_malloc(sizeof(double) * ((size_t) ld + u->m));
        u->cap = (u->d_x && u->h_buf) ? (int) n : 0;
    }
    if (u->cap >= (int) n && m == u->m) {
        memcpy(u->h_buf, x, sizeof(double) * n);
        if (!(nla_memcpy_h2d(u->d_x, u->h_buf, sizeof(double) * n, u->st) ||
              nla_usercon_eval_rows(u, (int) n, ld, 1, u->d_x, (int) u->m, u->d_c, u->st) ||
              nla_memcpy_d2h(u->h_buf + ld, u->d_c, sizeof(double) * u->m, u->st) || nla_stream_sync(u->st))) {
            memcpy(result, u->h_buf + ld, sizeof(double) * m);
            ok = 1;
        }
    }
    pthread_mutex_unlock(&u->lock);
    if (!ok) for (j = 0; j < m; ++j) result[j] = HUGE_VAL;
}
int nla_usercon_is_adapter(nlopt_mfunc mf) { return mf == adapter; }
nla_usercon *nla_usercon_of(const nla_constraint *c) { return c && c->mf == adapter ? (nla_usercon *) c->f_data : NULL; }
unsigned nla_usercon_m(const nla_usercon *u) { return u ? u->m : 0; }

/* the values of constraint entry `index` (of the inequality or the equality list) at x, through the entry's own callback — what
 * every host path gets; for a bound block without a twin that is one point through its kernel.  0, or -1: no such entry.  (tests) */
int nla_constraint_eval(const nlopt_opt opt, int equality, unsigned index, unsigned n, const double *x, double *result)
{
    const nla_constraint *c;
    if (!opt || !x || !result || index >= (equality ? opt->p : opt->m)) return -1;
    c = (equality ? opt->h : opt->fc) + index;
    if (c->f) result[0] = c->f(n, x, NULL, c->f_data);
    else c->mf(c->m, result, n, x, NULL, c->f_data);
    return 0;
}

static nlopt_result bind(nlopt_opt opt, int equality, unsigned m, const char *code_object, const char *name, nlopt_mfunc twin, void *data,
                         const double *tol, const void *dev_data, size_t dev_bytes)
{
    nla_usercon *u;
    char sym[256];
    nlopt_result r;
    if (!opt) return NLOPT_INVALID_ARGS;
    nla_unset_errmsg(opt);
    if (!code_object || !name || strlen(name) > 200 || m == 0) {
        nla_set_errmsg(opt, "nlopt_amd: device constraints need a code object path, a name and m > 0");
        return NLOPT_INVALID_ARGS;
    }
    if (!dev_data && dev_bytes > 0) { nla_set_errmsg(opt, "nlopt_amd: device constraint data is NULL with bytes > 0"); return NLOPT_INVALID_ARGS; }
    if (nla_dev_count() <= 0) { nla_set_errmsg(opt, "nlopt_amd: no HIP device visible (this library has no CPU fallback)"); return NLOPT_FAILURE; }
    u = (nla_usercon *) calloc(1, sizeof *u);
    if (!u) return NLOPT_OUT_OF_MEMORY;
    u->refs = 1; u->m = m; u->twin = twin; u->twin_data = data;
    pthread_mutex_init(&u->lock, NULL);
    if (!(u->module = nla_module_load_file(code_object))) {
        nla_set_errmsg(opt, "nlopt_amd: could not load code object %s (build it for gfx950 with hipcc --genco)", code_object);
        nla_usercon_release(u); return NLOPT_INVALID_ARGS;
    }
    /* either ABI's kernel must be there (the ABI-1 name first: its message is the one such code objects have always got) */
    snprintf(sym, sizeof sym, "%s_coneval", name);
    if (!(u->fn = nla_module_function(u->module, sym))) {
        char sym_d[256];
        snprintf(sym_d, sizeof sym_d, "%s_coneval_d", name);
        if (!nla_module_function(u->module, sym_d)) {
            nla_set_errmsg(opt, "nlopt_amd: kernel %s not found in %s (NLOPT_AMD_DEVICE_CONSTRAINTS(%s, ...) of nlopt_amd_device.h defines it)", sym, code_object, name);
            nla_usercon_release(u); return NLOPT_INVALID_ARGS;
        }
    }
    u->st = nla_stream_create();
    u->d_c = (double *) nla_dev_malloc(sizeof(double) * m);
    if (!u->st || !u->d_c) { nla_usercon_release(u); return NLOPT_OUT_OF_MEMORY; }
    {   /* ABI check: <name>_conabi writes the header's version: 1 -> <name>_coneval, 2 -> <name>_coneval_d */
        void *abi;
        int32_t *d_v = (int32_t *) nla_dev_malloc(sizeof(int32_t)), v = -1;
        void *params[1];
        snprintf(sym, sizeof sym, "%s_conabi", name);
        abi = nla_module_function(u->module, sym);
        params[0] = &d_v;
        if (!abi || !d_v || nla_module_launch(abi, 1, 1, params, u->st) || nla_memcpy_d2h(&v, d_v, sizeof v, u->st) || nla_stream_sync(u->st)) v = -1;
        nla_dev_free(d_v);
        if (v == 2) {
            snprintf(sym, sizeof sym, "%s_coneval_d", name);
            u->fn = nla_module_function(u->module, sym);
        }
        if ((v != 1 && v != 2) || !u->fn) {
            nla_set_errmsg(opt, "nlopt_amd: %s in %s was not built with this library's nlopt_amd_device.h (ABI %d, expected 1)", name, code_object, (int) v);
            nla_usercon_release(u); return NLOPT_INVALID_ARGS;
        }
        u->abi = v;
    }
    if (dev_bytes > 0) {
        if (u->abi < 2) {
            nla_set_errmsg(opt, "nlopt_amd: the constraint block %s is ABI 1 and takes no data (NLOPT_AMD_DEVICE_CONSTRAINTS_DATA of nlopt_amd_device.h does)", name);
            nla_usercon_release(u); return NLOPT_INVALID_ARGS;
        }
        /* copied now (synchronously: the caller may free its buffer on return) into memory the block owns */
        if (!(u->d_data = nla_dev_malloc(dev_bytes)) || nla_memcpy_h2d(u->d_data, dev_data, dev_bytes, u->st) || nla_stream_sync(u->st)) {
            nla_set_errmsg(opt, "nlopt_amd: could not copy %zu bytes of constraint data to the device", dev_bytes);
            nla_usercon_release(u); return NLOPT_OUT_OF_MEMORY;
        }
        u->data_bytes = dev_bytes;
    }
    /* the reference's checks and tolerance handling; the appended entry takes its own reference (api_options.c, push_constraint), so this
     * function's goes either way — refused, the block is freed here */
    r = equality ? nlopt_add_equality_mconstraint(opt, m, adapter, u, tol) : nlopt_add_inequality_mconstraint(opt, m, adapter, u, tol);
    nla_usercon_release(u);
    return r;
}

nlopt_result nlopt_amd_add_inequality_device_mconstraint(nlopt_opt opt, unsigned m, const char *code_object, const char *name,
                                                         nlopt_mfunc host_twin, void *data, const double *tol)
{ return bind(opt, 0, m, code_object, name, host_twin, data, tol, NULL, 0); }
nlopt_result nlopt_amd_add_equality_device_mconstraint(nlopt_opt opt, unsigned m, const char *code_object, const char *name,
                                                       nlopt_mfunc host_twin, void *data, const double *tol)
{ return bind(opt, 1, m, code_object, name, host_twin, data, tol, NULL, 0); }
/* the same with `dev_bytes` bytes of the caller's for the block's ABI-2 kernel (<name>_coneval_d), copied at the call */
nlopt_result nlopt_amd_add_inequality_device_mconstraint_data(nlopt_opt opt, unsigned m, const char *code_object, const char *name,
                                                              nlopt_mfunc host_twin, void *twin_data, const double *tol, const void *dev_data,
                                                              size_t dev_bytes)
{ return bind(opt, 0, m, code_object, name, host_twin, twin_data, tol, dev_data, dev_bytes); }
nlopt_result nlopt_amd_add_equality_device_mconstraint_data(nlopt_opt opt, unsigned m, const char *code_object, const char *name,
                                                            nlopt_mfunc host_twin, void *twin_data, const double *tol, const void *dev_data,
                                                            size_t dev_bytes)
{ return bind(opt, 1, m, code_object, name, host_twin, twin_data, tol, dev_data, dev_bytes); }
int nlopt_amd_device_constraint_count(const nlopt_opt opt)
{
    unsigned i;
    int c = 0;
    if (!opt) return 0;
    for (i = 0; i < opt->m; ++i) c += nla_usercon_of(opt->fc + i) != NULL;
    for (i = 0; i < opt->p; ++i) c += nla_usercon_of(opt->h + i) != NULL;
    return c;
}
