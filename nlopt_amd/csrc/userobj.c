/* userobj.c — user-supplied device objectives (include/nlopt_amd.h part 1, include/nlopt_amd_device.h).
 *
 * The reference has no counterpart: its objective is a host callback (src/api/nlopt.h:60-62).  SURVEY.md §8b names "an
 * additive setter" as the extension a GPU implementation needs; this is it.  A bound objective is a loaded code object
 * and its <name>_evalgrad kernel (ABI 1) or <name>_evalgrad_d kernel (ABI 2: it also reads the optimiser's data block,
 * nlopt_amd_set_device_objective_data) or <name>_evalgrad_r kernel (ABI 3: each candidate reads its own data ROW,
 * nlopt_amd_set_device_objective_row_data; served by nlopt_amd_optimize_batch alone, batch_driver.c — launch() below refuses to reach
 * past the rows that were set); the algorithms reach it through nla_evaluator (kind NLA_EVAL_USER).  What they hold is the
 * OPTIMISER's nla_userobj — its share of the loaded kernel plus its own data — so every launch below passes that optimiser's data:
 *   populations / samples   nla_userobj_eval_rows     one launch over all rows, one wavefront per row
 *   local searches          nla_userobj_evalgrad_list  one launch per step over the searches that wait (local_ctx.c)
 *   anything else           the adapter callback below: a single point through the same kernel (exact, slow) */
#include "nla_internal.h"
#include <math.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* the loaded kernel and the single-point scratch: ONE per binding, shared by every nlopt_copy of the optimiser it was bound to */
typedef struct {
    int refs;
    void *module, *fn;
    int abi;                               /* 1: <name>_evalgrad; 2: <name>_evalgrad_d, which also takes the data block; 3: <name>_evalgrad_r, a data row per candidate */
    int form, np;                          /* ABI 2, <name>_form: 0 one wavefront per candidate; 1 residual sums, one workgroup per candidate, n <= np */
    nlopt_func twin; void *twin_data;
    /* single-point evaluation through the kernel (adapter): one scratch set per binding — and the binding is shared by nlopt_copy
     * (per-thread copies are the normal NLopt pattern), so the adapter serialises on `lock` */
    pthread_mutex_t lock;
    void *st;
    double *d_x, *d_g, *d_f, *h_buf;       /* h_buf pinned: x | g | f */
    int cap;
} usercore;

/* the caller's data in device memory: immutable once made, reference counted, shared by nlopt_copy until one side sets data anew */
typedef struct { int refs; void *d; size_t bytes; size_t rows, row_stride; } userdata;     /* ABI 3: `rows` blocks of `bytes`, row_stride apart */

/* what an nlopt_opt owns (opt->userobj, and the f_data of its adapter callback): its share of the binding and ITS data block */
struct nla_userobj {
    usercore *core;
    userdata *data;
};

static void core_release(usercore *u)
{
    if (!u || __atomic_sub_fetch(&u->refs, 1, __ATOMIC_ACQ_REL) > 0) return;
    if (u->st) nla_stream_sync(u->st);
    nla_dev_free(u->d_x); nla_dev_free(u->d_g); nla_dev_free(u->d_f); nla_host_free(u->h_buf);
    if (u->st) nla_stream_destroy(u->st);
    nla_module_unload(u->module);
    pthread_mutex_destroy(&u->lock);
    free(u);
}
static void data_release(userdata *d)
{
    if (!d || __atomic_sub_fetch(&d->refs, 1, __ATOMIC_ACQ_REL) > 0) return;
    nla_dev_free(d->d);
    free(d);
}
/* `bytes` bytes of the caller's copied into device memory (synchronously: the caller may free its buffer on return); NULL: failed */
static userdata *data_create(const void *src, size_t bytes)
{
    userdata *d = (userdata *) calloc(1, sizeof *d);
    void *st = d ? nla_stream_create() : NULL;
    if (d && st && (d->d = nla_dev_malloc(bytes)) && !nla_memcpy_h2d(d->d, src, bytes, st) && !nla_stream_sync(st)) {
        d->refs = 1; d->bytes = bytes;
    } else if (d) { nla_dev_free(d->d); free(d); d = NULL; }
    if (st) nla_stream_destroy(st);
    return d;
}

/* `rows` blocks of row_bytes (contiguous at src) copied `stride` bytes apart (the padding zeroed); NULL: failed */
static userdata *data_create_rows(const void *src, size_t rows, size_t row_bytes, size_t stride)
{
    userdata *d = (userdata *) calloc(1, sizeof *d);
    void *st = d ? nla_stream_create() : NULL;
    /* staged through one padded host image: one copy, whatever the number of rows */
    char *img = d && st ? (char *) calloc(rows, stride) : NULL;
    size_t r;
    if (img) for (r = 0; r < rows; ++r) memcpy(img + r * stride, (const char *) src + r * row_bytes, row_bytes);
    if (img && (d->d = nla_dev_malloc(rows * stride)) && !nla_memcpy_h2d(d->d, img, rows * stride, st) && !nla_stream_sync(st)) {
        d->refs = 1; d->bytes = row_bytes; d->rows = rows; d->row_stride = stride;
    } else if (d) { nla_dev_free(d->d); free(d); d = NULL; }
    free(img);
    if (st) nla_stream_destroy(st);
    return d;
}

/* the copy's own share of u's binding and data (nlopt_copy) */
nla_userobj *nla_userobj_clone(const nla_userobj *u)
{
    nla_userobj *c;
    if (!u || !(c = (nla_userobj *) calloc(1, sizeof *c))) return NULL;
    *c = *u;
    __atomic_add_fetch(&c->core->refs, 1, __ATOMIC_RELAXED);
    if (c->data) __atomic_add_fetch(&c->data->refs, 1, __ATOMIC_RELAXED);
    return c;
}
void nla_userobj_release(nla_userobj *u)
{
    if (!u) return;
    data_release(u->data);
    core_release(u->core);
    free(u);
}

static int launch(nla_userobj *v, int n, int ld, int64_t count, const int32_t *list, const double *X, double *F, double *G, double sign,
                  int64_t row0, int64_t span, void *stream)
{
    /* <name>_evalgrad(int n, int ld, long count, const int *list, const double *X, double *F, double *G, double sign)
     * <name>_evalgrad_d(the same, const void *data, size_t data_bytes)
     * <name>_evalgrad_r(the same, const void *data, size_t row_bytes, size_t row_stride, long row0): row r of X reads data row row0 + r;
     *                   the rows of X a launch may name are 0 .. span - 1 (list == NULL: span = count) */
    const usercore *u = v->core;
    int32_t an = n, ald = ld;
    int64_t acount = count, arow0 = row0;
    double asign = sign == 0. ? 1. : sign;
    const void *adata = v->data ? v->data->d : NULL;
    size_t abytes = v->data ? v->data->bytes : 0, astride = v->data ? v->data->row_stride : 0;
    void *params[12];
    if (count <= 0) return 0;
    /* a row-data kernel cannot check the row it is handed: no launch may reach past the rows that were set */
    if (u->abi == 3 && (row0 < 0 || span < count || (uint64_t) row0 + (uint64_t) span > (uint64_t) (v->data ? v->data->rows : 0))) return -1;
    params[0] = &an; params[1] = &ald; params[2] = &acount; params[3] = &list; params[4] = &X; params[5] = &F; params[6] = &G; params[7] = &asign;
    params[8] = &adata; params[9] = &abytes;       /* (ABI 1 takes the first eight) */
    params[10] = &astride; params[11] = &arow0;    /* (ABI 3) */
    if (u->abi >= 2 && u->form == 1) {
        if (n > u->np || count > 0x7fffffff) return -1;      /* the residual kernel holds x in NP registers; one workgroup per candidate */
        return nla_module_launch(u->fn, (unsigned) count, 256, params, stream);
    }
    return nla_module_launch(u->fn, (unsigned) ((count + 3) / 4), 256, params, stream);
}

int nla_userobj_eval_rows(nla_userobj *u, int n, int ld, int64_t count, const double *X, double *F, double *G, double sign, void *stream)
{
    return launch(u, n, ld, count, NULL, X, F, G, sign, 0, count, stream);
}
int nla_userobj_evalgrad_list_rows(nla_userobj *u, int n, int ld, int m, const int32_t *d_list, const double *X, double *F, double *G,
                                   double sign, int64_t row0, int64_t span, void *stream)
{
    return launch(u, n, ld, m, d_list, X, F, G, sign, row0, span, stream);
}
int64_t nla_userobj_data_rows(const nla_userobj *u)
{
    return !u || u->core->abi != 3 ? -1 : u->data ? (int64_t) u->data->rows : 0;
}
int nla_userobj_evalgrad_list(nla_userobj *u, int n, int ld, int m, const int32_t *d_list, const double *X, double *F, double *G,
                              double sign, void *stream)
{
    return launch(u, n, ld, m, d_list, X, F, G, sign, 0, m, stream);
}

/* the objective as an ordinary nlopt_func: the host twin if the user gave one, else one point through the kernel — with the data of
 * the optimiser whose callback this is (`data` is that optimiser's nla_userobj) */
static double adapter(unsigned n, const double *x, double *grad, void *data)
{
    nla_userobj *v = (nla_userobj *) data;
    usercore *u = v->core;
    const int ld = (int) ((n + 1) & ~1u);
    double fv = HUGE_VAL;
    if (u->twin) return u->twin(n, x, grad, u->twin_data);
    if (u->abi == 3) return fv;                /* a row-data objective has no single block to evaluate a lone point on (nlopt_optimize refuses it) */
    pthread_mutex_lock(&u->lock);
    if ((int) n > u->cap) {
        nla_dev_free(u->d_x); nla_dev_free(u->d_g); nla_host_free(u->h_buf);
        u->d_x = (double *) nla_dev_malloc(sizeof(double) * (size_t) ld);
        u->d_g = (double *) nla_dev_malloc(sizeof(double) * (size_t) ld);
        u->h_buf = (double *) nla_host_malloc(sizeof(double) * (2 * (size_t) ld + 1));
        u->cap = (u->d_x && u->d_g && u->h_buf) ? (int) n : 0;
    }
    if (u->cap >= (int) n) {
        memcpy(u->h_buf, x, sizeof(double) * n);
        if (!(nla_memcpy_h2d(u->d_x, u->h_buf, sizeof(double) * n, u->st) ||
              launch(v, (int) n, ld, 1, NULL, u->d_x, u->d_f, grad ? u->d_g : NULL, 1., 0, 1, u->st) ||
              nla_memcpy_d2h(u->h_buf + 2 * (size_t) ld, u->d_f, sizeof(double), u->st) ||
              (grad && nla_memcpy_d2h(u->h_buf + ld, u->d_g, sizeof(double) * n, u->st)) || nla_stream_sync(u->st))) {
            if (grad) memcpy(grad, u->h_buf + ld, sizeof(double) * n);
            fv = u->h_buf[2 * (size_t) ld];
        }
    }
    pthread_mutex_unlock(&u->lock);
    return fv;
}
int nla_userobj_is_adapter(nlopt_func f) { return f == adapter; }

/* runs the one-thread kernel `sym`(int *out) of the module and reads `count` ints back; 0, or -1: no such kernel / the launch failed */
static int read_ints(usercore *u, const char *sym, int32_t *out, int count)
{
    void *k = nla_module_function(u->module, sym);
    int32_t *d_v = k ? (int32_t *) nla_dev_malloc(sizeof(int32_t) * (size_t) count) : NULL;
    void *params[1];
    int bad;
    params[0] = &d_v;
    bad = !k || !d_v || nla_module_launch(k, 1, 1, params, u->st) || nla_memcpy_d2h(out, d_v, sizeof(int32_t) * (size_t) count, u->st) || nla_stream_sync(u->st);
    nla_dev_free(d_v);
    return bad ? -1 : 0;
}

static nlopt_result bind(nlopt_opt opt, const char *code_object, const char *name, nlopt_func twin, void *f_data, int maximize)
{
    usercore *u;
    nla_userobj *v;
    char sym[256];
    int32_t abi = -1, form[2] = { 0, 0 };
    nlopt_result r;
    if (!opt) return NLOPT_INVALID_ARGS;
    nla_unset_errmsg(opt);
    if (!code_object || !name || strlen(name) > 200) { nla_set_errmsg(opt, "nlopt_amd: device objective needs a code object path and a name"); return NLOPT_INVALID_ARGS; }
    if (nla_dev_count() <= 0) { nla_set_errmsg(opt, "nlopt_amd: no HIP device visible (this library has no CPU fallback)"); return NLOPT_FAILURE; }
    u = (usercore *) calloc(1, sizeof *u);
    if (!u) return NLOPT_OUT_OF_MEMORY;
    u->refs = 1; u->twin = twin; u->twin_data = f_data;
    pthread_mutex_init(&u->lock, NULL);
    if (!(u->module = nla_module_load_file(code_object))) {
        nla_set_errmsg(opt, "nlopt_amd: could not load code object %s (build it for gfx950 with hipcc --genco)", code_object);
        core_release(u); return NLOPT_INVALID_ARGS;
    }
    /* either ABI's kernel must be there (an ABI-1 name is looked up first: its message is the one such code objects have always got) */
    snprintf(sym, sizeof sym, "%s_evalgrad", name);
    if (!(u->fn = nla_module_function(u->module, sym))) {
        char sym_d[256];
        char sym_r[256];
        snprintf(sym_d, sizeof sym_d, "%s_evalgrad_d", name);
        snprintf(sym_r, sizeof sym_r, "%s_evalgrad_r", name);
        if (!nla_module_function(u->module, sym_d) && !nla_module_function(u->module, sym_r)) {
            nla_set_errmsg(opt, "nlopt_amd: kernel %s not found in %s (NLOPT_AMD_DEVICE_OBJECTIVE(%s, ...) of nlopt_amd_device.h defines it)", sym, code_object, name);
            core_release(u); return NLOPT_INVALID_ARGS;
        }
    }
    u->st = nla_stream_create();
    u->d_f = (double *) nla_dev_malloc(sizeof(double));
    if (!u->st || !u->d_f) { core_release(u); return NLOPT_OUT_OF_MEMORY; }
    /* ABI check: <name>_abi writes the header's version: 1 -> <name>_evalgrad, 2 -> <name>_evalgrad_d and <name>_form */
    snprintf(sym, sizeof sym, "%s_abi", name);
    if (read_ints(u, sym, &abi, 1)) abi = -1;
    if (abi == 2 || abi == 3) {
        snprintf(sym, sizeof sym, abi == 3 ? "%s_evalgrad_r" : "%s_evalgrad_d", name);
        u->fn = nla_module_function(u->module, sym);
        snprintf(sym, sizeof sym, "%s_form", name);
        if (!u->fn || read_ints(u, sym, form, 2) || form[0] < 0 || form[0] > 1 || (form[0] == 1 && (form[1] < 1 || form[1] > 32))) {
            if (abi == 3)
                nla_set_errmsg(opt, "nlopt_amd: %s in %s reports ABI 3 but lacks a usable %s_evalgrad_r / %s_form (the ..._OBJECTIVE_ROWS / _RESIDUALS_ROWS macros of nlopt_amd_device.h define both)",
                               name, code_object, name, name);
            else
            nla_set_errmsg(opt, "nlopt_amd: %s in %s reports ABI 2 but lacks a usable %s_evalgrad_d / %s_form (the ..._DATA / _RESIDUALS macros of nlopt_amd_device.h define both)",
                           name, code_object, name, name);
            core_release(u); return NLOPT_INVALID_ARGS;
        }
        u->form = form[0]; u->np = form[1];
        if (u->form == 1 && (int) opt->n > u->np) {
            nla_set_errmsg(opt, "nlopt_amd: the residual objective %s serves n <= %d (NLOPT_AMD_DEVICE_RESIDUALS(%s, ..., %d)), this optimiser has n = %u",
                           name, u->np, name, u->np, opt->n);
            core_release(u); return NLOPT_INVALID_ARGS;
        }
    } else if (abi != 1 || !u->fn) {
        nla_set_errmsg(opt, "nlopt_amd: %s in %s was not built with this library's nlopt_amd_device.h (ABI %d, expected 1)", name, code_object, (int) abi);
        core_release(u); return NLOPT_INVALID_ARGS;
    }
    u->abi = abi;
    if (!(v = (nla_userobj *) calloc(1, sizeof *v))) { core_release(u); return NLOPT_OUT_OF_MEMORY; }
    v->core = u;
    r = maximize ? nlopt_set_max_objective(opt, adapter, v) : nlopt_set_min_objective(opt, adapter, v);   /* releases a previous binding (and its data) */
    if (r != NLOPT_SUCCESS) { nla_userobj_release(v); return r; }
    opt->userobj = v;
    return NLOPT_SUCCESS;
}

nlopt_result nlopt_amd_set_min_device_objective(nlopt_opt opt, const char *code_object, const char *name, nlopt_func host_twin, void *f_data)
{ return bind(opt, code_object, name, host_twin, f_data, 0); }
nlopt_result nlopt_amd_set_max_device_objective(nlopt_opt opt, const char *code_object, const char *name, nlopt_func host_twin, void *f_data)
{ return bind(opt, code_object, name, host_twin, f_data, 1); }
int nlopt_amd_has_device_objective(const nlopt_opt opt) { return opt && opt->userobj ? 1 : 0; }

/* the data the bound ABI-2 objective reads: copied now, owned by THIS optimiser (a copy made later shares the block; setting data on
 * either side afterwards replaces that side's block only) */
nlopt_result nlopt_amd_set_device_objective_data(nlopt_opt opt, const void *data, size_t bytes)
{
    userdata *d = NULL;
    if (!opt) return NLOPT_INVALID_ARGS;
    nla_unset_errmsg(opt);
    if (!opt->userobj) { nla_set_errmsg(opt, "nlopt_amd: no device objective is bound (nlopt_amd_set_min/max_device_objective comes first)"); return NLOPT_INVALID_ARGS; }
    if (opt->userobj->core->abi < 2) {
        nla_set_errmsg(opt, "nlopt_amd: the bound device objective is ABI 1 and takes no data (NLOPT_AMD_DEVICE_OBJECTIVE_DATA / _RESIDUALS of nlopt_amd_device.h do)");
        return NLOPT_INVALID_ARGS;
    }
    if (opt->userobj->core->abi == 3) {
        nla_set_errmsg(opt, "nlopt_amd: the bound device objective reads a data row per search (ABI 3): nlopt_amd_set_device_objective_row_data sets its data");
        return NLOPT_INVALID_ARGS;
    }
    if (!data && bytes > 0) { nla_set_errmsg(opt, "nlopt_amd: device objective data is NULL with bytes > 0"); return NLOPT_INVALID_ARGS; }
    if (bytes > 0 && !(d = data_create(data, bytes))) { nla_set_errmsg(opt, "nlopt_amd: could not copy %zu bytes of objective data to the device", bytes); return NLOPT_OUT_OF_MEMORY; }
    data_release(opt->userobj->data);
    opt->userobj->data = d;
    return NLOPT_SUCCESS;
}

/* the rows an ABI-3 objective reads: `rows` blocks of row_bytes copied now, 256-byte aligned each; owned like the block above */
nlopt_result nlopt_amd_set_device_objective_row_data(nlopt_opt opt, size_t rows, size_t row_bytes, const void *data)
{
    userdata *d = NULL;
    if (!opt) return NLOPT_INVALID_ARGS;
    nla_unset_errmsg(opt);
    if (!opt->userobj) { nla_set_errmsg(opt, "nlopt_amd: no device objective is bound (nlopt_amd_set_min/max_device_objective comes first)"); return NLOPT_INVALID_ARGS; }
    if (opt->userobj->core->abi != 3) {
        nla_set_errmsg(opt, "nlopt_amd: the bound device objective is ABI %d and takes no row data (NLOPT_AMD_DEVICE_OBJECTIVE_ROWS / _RESIDUALS_ROWS of nlopt_amd_device.h do)",
                       opt->userobj->core->abi);
        return NLOPT_INVALID_ARGS;
    }
    if (rows > 0 && (!data || row_bytes == 0)) { nla_set_errmsg(opt, "nlopt_amd: device objective row data is NULL or has row_bytes == 0 with rows > 0"); return NLOPT_INVALID_ARGS; }
    if (rows > 0) {
        const size_t stride = (row_bytes + 255) & ~(size_t) 255;
        if (stride < row_bytes || rows > (size_t) -1 / stride / 2) { nla_set_errmsg(opt, "nlopt_amd: device objective row data too large"); return NLOPT_INVALID_ARGS; }
        if (!(d = data_create_rows(data, rows, row_bytes, stride))) {
            nla_set_errmsg(opt, "nlopt_amd: could not copy %zu rows of %zu bytes of objective data to the device", rows, row_bytes);
            return NLOPT_OUT_OF_MEMORY;
        }
    }
    data_release(opt->userobj->data);
    opt->userobj->data = d;
    return NLOPT_SUCCESS;
}

/* f (and the gradient) of `count` host points through the bound kernel in one launch, sign +1: what a user checks a model with */
nlopt_result nlopt_amd_eval_device_objective(nlopt_opt opt, size_t count, const double *x, double *f, double *grad)
{
    nla_userobj *v;
    const size_t n = opt ? opt->n : 0, ld = (n + 1) & ~(size_t) 1;
    double *d_X = NULL, *d_F = NULL, *d_G = NULL, *h = NULL;
    void *st = NULL;
    size_t c;
    nlopt_result ret = NLOPT_FAILURE;
    if (!opt) return NLOPT_INVALID_ARGS;
    nla_unset_errmsg(opt);
    if (!(v = opt->userobj)) { nla_set_errmsg(opt, "nlopt_amd: no device objective is bound"); return NLOPT_INVALID_ARGS; }
    if (count == 0) return NLOPT_SUCCESS;
    if (!x || !f || n == 0 || count > 0x7fffffff) { nla_set_errmsg(opt, "nlopt_amd: eval_device_objective needs points, room for f, n > 0 and count < 2^31"); return NLOPT_INVALID_ARGS; }
    if (v->core->abi == 3 && count > (v->data ? v->data->rows : 0)) {
        nla_set_errmsg(opt, "nlopt_amd: the bound row-data objective evaluates point c on data row c: %zu points, %zu rows set (nlopt_amd_set_device_objective_row_data)",
                       count, v->data ? v->data->rows : (size_t) 0);
        return NLOPT_INVALID_ARGS;
    }
    if (v->core->abi >= 2 && v->core->form == 1 && (int) n > v->core->np) {
        nla_set_errmsg(opt, "nlopt_amd: the bound residual objective serves n <= %d", v->core->np);
        return NLOPT_INVALID_ARGS;
    }
    st = nla_stream_create();
    d_X = (double *) nla_dev_malloc(sizeof(double) * ld * count);
    d_F = (double *) nla_dev_malloc(sizeof(double) * count);
    if (grad) d_G = (double *) nla_dev_malloc(sizeof(double) * ld * count);
    h = (double *) malloc(sizeof(double) * ld * count);
    if (!st || !d_X || !d_F || (grad && !d_G) || !h) { ret = NLOPT_OUT_OF_MEMORY; goto done; }
    memset(h, 0, sizeof(double) * ld * count);
    for (c = 0; c < count; ++c) memcpy(h + c * ld, x + c * n, sizeof(double) * n);
    if (nla_memcpy_h2d(d_X, h, sizeof(double) * ld * count, st) ||
        launch(v, (int) n, (int) ld, (int64_t) count, NULL, d_X, d_F, d_G, 1., 0, (int64_t) count, st) ||
        nla_memcpy_d2h(f, d_F, sizeof(double) * count, st) || nla_stream_sync(st)) { nla_set_errmsg(opt, "nlopt_amd: user objective launch failed"); goto done; }
    if (grad) {
        if (nla_memcpy_d2h(h, d_G, sizeof(double) * ld * count, st) || nla_stream_sync(st)) { nla_set_errmsg(opt, "nlopt_amd: user objective launch failed"); goto done; }
        for (c = 0; c < count; ++c) memcpy(grad + c * n, h + c * ld, sizeof(double) * n);
    }
    ret = NLOPT_SUCCESS;
done:
    if (st) nla_stream_sync(st);
    nla_dev_free(d_X); nla_dev_free(d_F); nla_dev_free(d_G); free(h);
    if (st) nla_stream_destroy(st);
    return ret;
}

/* how an objective handed to an algorithm driver is to be evaluated */
void nla_evaluator_resolve(nla_evaluator *ev, nlopt_opt opt, nlopt_func f, void *f_data)
{
    memset(ev, 0, sizeof *ev);
    ev->f = f; ev->f_data = f_data;
    ev->sign = (opt && opt->dev_sign < 0) ? -1. : 1.;
    ev->obj = nlopt_amd_objective_id(f);
    if (ev->obj >= 0) ev->kind = NLA_EVAL_DEVICE;
    else if (f == adapter && f_data) { ev->kind = NLA_EVAL_USER; ev->user = (nla_userobj *) f_data; }
    else { ev->kind = NLA_EVAL_HOST; ev->sign = 1.; }
}

int nla_exact_mode(nlopt_opt opt) { return opt && nlopt_get_param(opt, "amd_exact_dot", 0.) != 0.; }

/* Which summation order a local search uses.  "amd_exact_dot" set on the object (or on MLSL's local optimiser, `also`) decides;
 * unset, a client's own nlopt_func gets the reference's sequential order — its callback sees exactly the points the reference
 * would hand it, which is what a drop-in owes it, and the callback's round trip dwarfs the cost of the ordered sums — while
 * device objectives get the tree reductions (results to rounding). */
int nla_exact_mode_for(nlopt_opt opt, nlopt_opt also, const nla_evaluator *ev)
{
    const int set_a = opt && nlopt_has_param(opt, "amd_exact_dot"), set_b = also && nlopt_has_param(also, "amd_exact_dot");
    int exact = (set_a || set_b) ? ((set_a && nla_exact_mode(opt)) || (set_b && nla_exact_mode(also))) : (ev && ev->kind == NLA_EVAL_HOST);
    /* "amd_lbfgs_streaming" != 0: LD_LBFGS with tree sums on the streaming kernel (hip/lbfgs_kernels.hip) instead of the resident one
     * (hip/lbfgs_resident.hip) — the two are bit-identical, which is what the switch exists to show (tests/test_gpu_lbfgs.py) */
    if ((opt && nlopt_get_param(opt, "amd_lbfgs_streaming", 0) != 0) || (also && nlopt_get_param(also, "amd_lbfgs_streaming", 0) != 0)) return exact ? 3 : 2;
    return exact;
}
