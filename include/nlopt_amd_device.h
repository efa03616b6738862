/* nlopt_amd_device.h — how a user puts an objective on the GPU for libnlopt_amd (HIP, gfx950).
 *
 * The reference's objective is a host callback (src/api/nlopt.h:60-62), which a GPU cannot call; SURVEY.md §8b lists "an
 * additive setter" for device objectives as the required extension.  This header is the device half of that extension:
 * the user describes the objective by its per-coordinate terms, the macro below turns the description into the one kernel
 * libnlopt_amd launches, the user compiles it into a code object
 *
 *     hipcc --offload-arch=gfx950 -O3 -ffp-contract=off --genco -I<libnlopt_amd>/include my_objective.hip -o my_objective.hsaco
 *
 * and binds it with nlopt_amd_set_min_device_objective(opt, "my_objective.hsaco", "myobj", host_twin, data)
 * (include/nlopt_amd.h).  No other file of the library is needed to compile it.
 *
 * Contract (the same as the compiled-in objectives, nlopt_amd/csrc/hip/dev_common.h): ONE WAVEFRONT (64 lanes) evaluates
 * one candidate.  An objective is described as
 *
 *     f(x) = finish(n, A, B, x)   with   A = sum_i a_i(x),  B = sum_i b_i(x)     (B a product if B_IS_PRODUCT)
 *     df/dx_i = grad(n, i, x, A, B)
 *
 *   struct MyObj {
 *       static constexpr bool B_IS_PRODUCT = false;
 *       __device__ static void terms(int n, int i, const double *x, double *a, double *b);    // a_i, b_i  (i < n)
 *       __device__ static double finish(int n, double A, double B, const double *x);
 *       __device__ static double grad(int n, int i, const double *x, double A, double B);
 *   };
 *   NLOPT_AMD_DEVICE_OBJECTIVE(myobj, MyObj)
 *
 * Lane l accumulates the terms of coordinates l, l+64, ... in that order; the 64 partial pairs are combined by a
 * xor-butterfly.  Only the association order of that reduction differs from a sequential host loop over the same terms, so
 * f agrees with a host twin written from the same formulas to rounding (1e-10 relative is the library's parity bar).
 * Compile with -ffp-contract=off if the host twin is.
 *
 * Kernel ABI (what the library launches; <name>_evalgrad, 64 x 4 threads per workgroup, one wavefront per candidate):
 *   (int n, int ld, long count, const int *list, const double *X, double *F, double *G, double sign)
 *   list == NULL: candidates are rows 0 .. count-1 of X (ld doubles apart): F[c] = sign f(row c); if G: row c of G =
 *   sign grad.  list != NULL: candidate c is row i with e = list[c], i = e >= 0 ? e : -(e+1); its gradient is wanted iff
 *   e >= 0; results go to F[i] and row i of G.
 */
#ifndef NLOPT_AMD_DEVICE_H
#define NLOPT_AMD_DEVICE_H

#include <hip/hip_runtime.h>

#define NLOPT_AMD_DEVICE_ABI 1

namespace nlopt_amd_device {

template <class OBJ>
__device__ __forceinline__ void evalgrad_wave(int n, const double *x, double *f_out, double *g, double sign)
{
    const int lane = threadIdx.x & 63;
    double A = 0, B = OBJ::B_IS_PRODUCT ? 1 : 0;
    for (int i = lane; i < n; i += 64) {
        double a, b;
        OBJ::terms(n, i, x, &a, &b);
        A += a;
        if (OBJ::B_IS_PRODUCT) B *= b; else B += b;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double oa = __shfl_xor(A, m, 64), ob = __shfl_xor(B, m, 64);
        A += oa;
        if (OBJ::B_IS_PRODUCT) B *= ob; else B += ob;
    }
    const double f = OBJ::finish(n, A, B, x);
    if (lane == 0) *f_out = sign * f;
    if (g) for (int i = lane; i < n; i += 64) g[i] = sign * OBJ::grad(n, i, x, A, B);
}

template <class OBJ>
__device__ __forceinline__ void evalgrad_kernel_body(int n, int ld, long count, const int *list, const double *X, double *F, double *G,
                                                     double sign)
{
    const long c = (long) blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (c >= count) return;
    long row = c;
    bool wantg = G != nullptr;
    if (list) { const int e = list[c]; row = e >= 0 ? e : -(long) e - 1; wantg = wantg && e >= 0; }
    evalgrad_wave<OBJ>(n, X + row * (long) ld, F + row, wantg ? G + row * (long) ld : nullptr, sign);
}

/* ---- nonlinear constraints (NLOPT_GN_ISRES; bound with nlopt_amd_add_inequality_device_mconstraint /
 * nlopt_amd_add_equality_device_mconstraint of include/nlopt_amd.h) ----------------------------------------------------------
 * A block of m constraints is described by its values:
 *
 *   struct MyCons {
 *       // value of constraint j (0 <= j < m) at x; plain sequential C++, called by ONE lane
 *       __device__ static double value(int n, int j, const double *x);
 *   };
 *   NLOPT_AMD_DEVICE_CONSTRAINTS(mycons, MyCons)
 *
 * Contract: one wavefront takes one candidate; lane j % 64 evaluates constraint j, alone and in program order (no reduction
 * across lanes).  A host twin written from the same formulas and compiled with -ffp-contract=off therefore gives the same bits as
 * long as the formulas use + - * / and sqrt only; the device's and the host's libm transcendentals (exp, sin, pow, ...) may differ
 * in the last places.
 *
 * Kernel ABI (<name>_coneval, 64 x 4 threads per workgroup, one wavefront per candidate):
 *   (int n, int ld, long count, const double *X, int m, int ldc, double *C)
 *   C[row * ldc + j] = value(n, j, X + row * ld) for row < count, j < m.  <name>_conabi(int *out) writes the ABI version; it is
 *   separate from <name>_abi, so one code object may hold an objective and a constraint block under the same name. */
template <class CON>
__device__ __forceinline__ void coneval_kernel_body(int n, int ld, long count, const double *X, int m, int ldc, double *C)
{
    const int lane = threadIdx.x & 63;
    const long row = (long) blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= count) return;
    const double *x = X + row * (long) ld;
    for (int j = lane; j < m; j += 64) C[row * (long) ldc + j] = CON::value(n, j, x);
}

}  // namespace nlopt_amd_device

#define NLOPT_AMD_DEVICE_CONSTRAINTS(name, CON)                                                                                \
    extern "C" __global__ __launch_bounds__(256) void name##_coneval(int n, int ld, long count, const double *X, int m,        \
                                                                     int ldc, double *C)                                       \
    { nlopt_amd_device::coneval_kernel_body<CON>(n, ld, count, X, m, ldc, C); }                                                \
    extern "C" __global__ void name##_conabi(int *out) { *out = NLOPT_AMD_DEVICE_ABI; }

#define NLOPT_AMD_DEVICE_OBJECTIVE(name, OBJ)                                                                                  \
    extern "C" __global__ __launch_bounds__(256) void name##_evalgrad(int n, int ld, long count, const int *list,              \
                                                                      const double *X, double *F, double *G, double sign)     \
    { nlopt_amd_device::evalgrad_kernel_body<OBJ>(n, ld, count, list, X, F, G, sign); }                                       \
    extern "C" __global__ void name##_abi(int *out) { *out = NLOPT_AMD_DEVICE_ABI; }

/* ==== ABI 2: objectives and constraints that read the caller's data =========================================================
 * The kernels of ABI 2 take two trailing arguments, (const void *data, size_t data_bytes): the block of bytes the caller handed to
 * nlopt_amd_set_device_objective_data (objectives) or nlopt_amd_add_*_device_mconstraint_data (constraints), copied into device
 * memory the library owns.  `data` is a device pointer, 256-byte aligned and read-only for the kernel, or (NULL, 0) when no data
 * was set.  <name>_abi / <name>_conabi write 2; the library tells the two ABIs apart by that value, and code objects built with
 * the ABI-1 macros above keep loading and run exactly as before.  One name carries ONE objective form.
 *
 * (a) NLOPT_AMD_DEVICE_OBJECTIVE_DATA(name, OBJ) — the terms / finish / grad form above with the data appended:
 *
 *   struct MyObj {
 *       static constexpr bool B_IS_PRODUCT = false;
 *       __device__ static void terms(int n, int i, const double *x, double *a, double *b, const void *data, size_t bytes);
 *       __device__ static double finish(int n, double A, double B, const double *x, const void *data, size_t bytes);
 *       __device__ static double grad(int n, int i, const double *x, double A, double B, const void *data, size_t bytes);
 *   };
 *
 *   Kernel <name>_evalgrad_d, (n, ld, count, list, X, F, G, sign, data, data_bytes); wavefront mapping, launch geometry and
 *   reduction order are those of ABI 1, so an objective that ignores its data gives the bits of its ABI-1 statement.
 *
 * (b) NLOPT_AMD_DEVICE_CONSTRAINTS_DATA(name, CON) — value(n, j, x, data, bytes); kernel <name>_coneval_d,
 *   (n, ld, count, X, m, ldc, C, data, data_bytes); lane mapping as in ABI 1.
 *
 * (c) NLOPT_AMD_DEVICE_RESIDUALS(name, RES, NP) — a sum over RESIDUALS instead of coordinates, the shape of a least-squares fit of a
 *   few parameters to many data points:
 *
 *       f(x) = sum_{k < m} r_k(x; data)^2          df/dx_i = 2 sum_k r_k dr_k/dx_i          n <= NP <= 32, NP a compile-time constant
 *
 *   struct MyFit {
 *       __device__ static long count(int n, const void *data, size_t bytes);                       // m, the same for every x
 *       template <bool GRAD>
 *       __device__ static double residual(int n, const double (&x)[NP], long k, const void *data, size_t bytes, double (&d)[NP]);
 *           // returns r_k; x[i] = 0 for i >= n.  GRAD: also d[i] = dr_k/dx_i for EVERY i < NP (0 for i >= n).  !GRAD: d is not read.
 *   };
 *
 *   Kernel <name>_evalgrad_d with the argument list of (a) and the meaning of `list` of ABI 1, but ONE WORKGROUP of 256 threads per
 *   candidate (the library launches `count` workgroups; <name>_form(int out[2]) tells it so: out[0] = the form, out[1] = NP, and
 *   the library refuses to launch the kernel with n > NP).  The order of the sums is fixed by m alone:
 *     per-thread sums  thread t (0..255) keeps x, one partial of f and NP partials of the gradient in registers and adds residuals
 *                      t, t+256, t+512, ... in that order:  f += r*r;  g[i] += r*d[i]
 *     butterfly        each of the four wavefronts combines its 64 partials with the xor-butterfly 32, 16, 8, 4, 2, 1
 *     wave combine     the four results meet in LDS as ((w0 + w1) + w2) + w3;  then F = sign * f,  G_i = sign * (2 * g_i)
 *   The split depends on nothing but m — never on count, list or the candidate's position in the launch — so the same point gives
 *   the same bits in a population launch, a list launch and a single-point launch.  m == 0 gives f = 0, g = 0.  The value computed
 *   with and without the gradient is the same as long as residual<true> and residual<false> return the same r_k.
 *   Write `residual` with compile-time indices into x and d (fully unrolled loops over NP): the arrays then live in registers. */
#define NLOPT_AMD_DEVICE_ABI_DATA 2
#define NLOPT_AMD_DEVICE_FORM_TERMS 0
#define NLOPT_AMD_DEVICE_FORM_RESIDUALS 1

namespace nlopt_amd_device {

template <class OBJ>
__device__ __forceinline__ void evalgrad_wave_d(int n, const double *x, double *f_out, double *g, double sign, const void *data, size_t bytes)
{
    const int lane = threadIdx.x & 63;
    double A = 0, B = OBJ::B_IS_PRODUCT ? 1 : 0;
    for (int i = lane; i < n; i += 64) {
        double a, b;
        OBJ::terms(n, i, x, &a, &b, data, bytes);
        A += a;
        if (OBJ::B_IS_PRODUCT) B *= b; else B += b;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double oa = __shfl_xor(A, m, 64), ob = __shfl_xor(B, m, 64);
        A += oa;
        if (OBJ::B_IS_PRODUCT) B *= ob; else B += ob;
    }
    const double f = OBJ::finish(n, A, B, x, data, bytes);
    if (lane == 0) *f_out = sign * f;
    if (g) for (int i = lane; i < n; i += 64) g[i] = sign * OBJ::grad(n, i, x, A, B, data, bytes);
}

/* the block candidate `row` reads: ABI 2 (row_stride == 0, row0 == 0) the one block every candidate shares; ABI 3 the block of data
 * row row0 + row, row_stride bytes apart */
__device__ __forceinline__ const void *row_data(const void *data, size_t row_stride, long row0, long row)
{
    return (const char *) data + (size_t) (row0 + row) * row_stride;
}

template <class OBJ>
__device__ __forceinline__ void evalgrad_kernel_body_rows(int n, int ld, long count, const int *list, const double *X, double *F, double *G,
                                                          double sign, const void *data, size_t bytes, size_t row_stride, long row0)
{
    const long c = (long) blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (c >= count) return;
    long row = c;
    bool wantg = G != nullptr;
    if (list) { const int e = list[c]; row = e >= 0 ? e : -(long) e - 1; wantg = wantg && e >= 0; }
    evalgrad_wave_d<OBJ>(n, X + row * (long) ld, F + row, wantg ? G + row * (long) ld : nullptr, sign,
                         row_data(data, row_stride, row0, row), bytes);
}

template <class OBJ>
__device__ __forceinline__ void evalgrad_kernel_body_d(int n, int ld, long count, const int *list, const double *X, double *F, double *G,
                                                       double sign, const void *data, size_t bytes)
{
    evalgrad_kernel_body_rows<OBJ>(n, ld, count, list, X, F, G, sign, data, bytes, 0, 0);
}

template <class CON>
__device__ __forceinline__ void coneval_kernel_body_d(int n, int ld, long count, const double *X, int m, int ldc, double *C,
                                                      const void *data, size_t bytes)
{
    const int lane = threadIdx.x & 63;
    const long row = (long) blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= count) return;
    const double *x = X + row * (long) ld;
    for (int j = lane; j < m; j += 64) C[row * (long) ldc + j] = CON::value(n, j, x, data, bytes);
}

/* the per-thread sums of one candidate: residuals t, t+256, ... in that order */
template <class RES, int NP, bool GRAD>
__device__ __forceinline__ void residual_thread_sums(int n, const double (&x)[NP], long m, const void *data, size_t bytes, double &f,
                                                     double (&g)[NP])
{
    double d[NP];
    for (long k = threadIdx.x; k < m; k += 256) {
        const double r = RES::template residual<GRAD>(n, x, k, data, bytes, d);
        f += r * r;
        if (GRAD) {
#pragma unroll
            for (int i = 0; i < NP; ++i) g[i] += r * d[i];
        }
    }
}

template <class RES, int NP>
__device__ __forceinline__ void residuals_kernel_body_rows(int n, int ld, long count, const int *list, const double *X, double *F, double *G,
                                                           double sign, const void *data_all, size_t bytes, size_t row_stride, long row0)
{
    static_assert(NP >= 1 && NP <= 32, "NLOPT_AMD_DEVICE_RESIDUALS serves 1 <= NP <= 32");
    __shared__ double part[4][NP + 1];
    const long c = blockIdx.x;                               /* one workgroup per candidate: everything below is uniform over it */
    if (c >= count || n > NP) return;
    long row = c;
    bool wantg = G != nullptr;
    if (list) { const int e = list[c]; row = e >= 0 ? e : -(long) e - 1; wantg = wantg && e >= 0; }
    const double *xr = X + row * (long) ld;
    const void *data = row_data(data_all, row_stride, row0, row);
    const int t = threadIdx.x, wave = t >> 6;
    double x[NP], g[NP], f = 0;
#pragma unroll
    for (int i = 0; i < NP; ++i) { x[i] = i < n ? xr[i] : 0.; g[i] = 0; }
    const long m = RES::count(n, data, bytes);
    if (wantg) residual_thread_sums<RES, NP, true>(n, x, m, data, bytes, f, g);
    else residual_thread_sums<RES, NP, false>(n, x, m, data, bytes, f, g);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) f += __shfl_xor(f, s, 64);
    if (wantg) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) g[i] += __shfl_xor(g[i], s, 64);
        }
    }
    if ((t & 63) == 0) {
        part[wave][0] = f;
        if (wantg) {
#pragma unroll
            for (int i = 0; i < NP; ++i) part[wave][1 + i] = g[i];
        }
    }
    __syncthreads();
    if (t == 0) F[row] = sign * (((part[0][0] + part[1][0]) + part[2][0]) + part[3][0]);
    if (wantg && t < n) G[row * (long) ld + t] = sign * (2 * (((part[0][1 + t] + part[1][1 + t]) + part[2][1 + t]) + part[3][1 + t]));
}

template <class RES, int NP>
__device__ __forceinline__ void residuals_kernel_body(int n, int ld, long count, const int *list, const double *X, double *F, double *G,
                                                      double sign, const void *data, size_t bytes)
{
    residuals_kernel_body_rows<RES, NP>(n, ld, count, list, X, F, G, sign, data, bytes, 0, 0);
}

}  // namespace nlopt_amd_device

#define NLOPT_AMD_DEVICE_OBJECTIVE_DATA(name, OBJ)                                                                             \
    extern "C" __global__ __launch_bounds__(256) void name##_evalgrad_d(int n, int ld, long count, const int *list,            \
                                                                        const double *X, double *F, double *G, double sign,   \
                                                                        const void *data, size_t data_bytes)                  \
    { nlopt_amd_device::evalgrad_kernel_body_d<OBJ>(n, ld, count, list, X, F, G, sign, data, data_bytes); }                   \
    extern "C" __global__ void name##_form(int *out) { out[0] = NLOPT_AMD_DEVICE_FORM_TERMS; out[1] = 0; }                    \
    extern "C" __global__ void name##_abi(int *out) { *out = NLOPT_AMD_DEVICE_ABI_DATA; }

#define NLOPT_AMD_DEVICE_CONSTRAINTS_DATA(name, CON)                                                                           \
    extern "C" __global__ __launch_bounds__(256) void name##_coneval_d(int n, int ld, long count, const double *X, int m,      \
                                                                       int ldc, double *C, const void *data,                  \
                                                                       size_t data_bytes)                                     \
    { nlopt_amd_device::coneval_kernel_body_d<CON>(n, ld, count, X, m, ldc, C, data, data_bytes); }                           \
    extern "C" __global__ void name##_conabi(int *out) { *out = NLOPT_AMD_DEVICE_ABI_DATA; }

#define NLOPT_AMD_DEVICE_RESIDUALS(name, RES, NP)                                                                              \
    extern "C" __global__ __launch_bounds__(256) void name##_evalgrad_d(int n, int ld, long count, const int *list,            \
                                                                        const double *X, double *F, double *G, double sign,   \
                                                                        const void *data, size_t data_bytes)                  \
    { nlopt_amd_device::residuals_kernel_body<RES, NP>(n, ld, count, list, X, F, G, sign, data, data_bytes); }                \
    extern "C" __global__ void name##_form(int *out) { out[0] = NLOPT_AMD_DEVICE_FORM_RESIDUALS; out[1] = NP; }               \
    extern "C" __global__ void name##_abi(int *out) { *out = NLOPT_AMD_DEVICE_ABI_DATA; }

/* ==== ABI 3: each candidate reads ITS OWN row of data =======================================================================
 * Many small problems of one shape — one curve per pixel, voxel or sensor — solved side by side by nlopt_amd_optimize_batch
 * (include/nlopt_amd.h): search i of the batch reads data row i.  The rows come from nlopt_amd_set_device_objective_row_data: `rows`
 * blocks of row_bytes bytes each, stored row_stride = round_up(row_bytes, 256) bytes apart, so every row keeps the 256-byte
 * alignment ABI 2 promises its one block.
 *
 *   NLOPT_AMD_DEVICE_OBJECTIVE_ROWS(name, OBJ)        OBJ: the struct NLOPT_AMD_DEVICE_OBJECTIVE_DATA takes, unchanged
 *   NLOPT_AMD_DEVICE_RESIDUALS_ROWS(name, RES, NP)    RES: the struct NLOPT_AMD_DEVICE_RESIDUALS takes, unchanged
 *
 * A model is written once and compiled under either macro (under different names).  Kernel <name>_evalgrad_r:
 *   (int n, int ld, long count, const int *list, const double *X, double *F, double *G, double sign,
 *    const void *data, size_t row_bytes, size_t row_stride, long row0)
 * The candidate in row r of X (r after `list` is resolved, as in ABI 1) hands the struct's functions
 *   ((const char *) data + (row0 + r) * row_stride, row_bytes).
 * Wavefront / workgroup mapping, per-thread sums, butterfly and wave combine are those of ABI 2 — the same function bodies with a
 * data pointer computed per row — so a search on data row k gives the bits of the ABI-2 kernel handed that block alone.  The
 * library guarantees row0 + r < rows for every candidate it launches.  <name>_abi writes 3; <name>_form as in ABI 2.
 * Out of scope: a block shared by all rows BESIDE the per-row block (one time axis, many signals). */
#define NLOPT_AMD_DEVICE_ABI_ROWS 3

#define NLOPT_AMD_DEVICE_OBJECTIVE_ROWS(name, OBJ)                                                                             \
    extern "C" __global__ __launch_bounds__(256) void name##_evalgrad_r(int n, int ld, long count, const int *list,            \
                                                                        const double *X, double *F, double *G, double sign,   \
                                                                        const void *data, size_t row_bytes,                   \
                                                                        size_t row_stride, long row0)                         \
    { nlopt_amd_device::evalgrad_kernel_body_rows<OBJ>(n, ld, count, list, X, F, G, sign, data, row_bytes, row_stride, row0); } \
    extern "C" __global__ void name##_form(int *out) { out[0] = NLOPT_AMD_DEVICE_FORM_TERMS; out[1] = 0; }                    \
    extern "C" __global__ void name##_abi(int *out) { *out = NLOPT_AMD_DEVICE_ABI_ROWS; }

#define NLOPT_AMD_DEVICE_RESIDUALS_ROWS(name, RES, NP)                                                                         \
    extern "C" __global__ __launch_bounds__(256) void name##_evalgrad_r(int n, int ld, long count, const int *list,            \
                                                                        const double *X, double *F, double *G, double sign,   \
                                                                        const void *data, size_t row_bytes,                   \
                                                                        size_t row_stride, long row0)                         \
    { nlopt_amd_device::residuals_kernel_body_rows<RES, NP>(n, ld, count, list, X, F, G, sign, data, row_bytes, row_stride,   \
                                                            row0); }                                                          \
    extern "C" __global__ void name##_form(int *out) { out[0] = NLOPT_AMD_DEVICE_FORM_RESIDUALS; out[1] = NP; }               \
    extern "C" __global__ void name##_abi(int *out) { *out = NLOPT_AMD_DEVICE_ABI_ROWS; }

#endif /* NLOPT_AMD_DEVICE_H */
