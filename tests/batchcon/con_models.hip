/* con_models.hip — what a user of include/nlopt_amd_device.h writes for a batch of small CONSTRAINED fits (nlopt_amd_optimize_batch with
 * NLOPT_LN_COBYLA): one objective family and a handful of constraint blocks, + - x only, so that every value is the same bits wherever
 * it is computed.  Built with
 *     hipcc --offload-arch=gfx950 -O3 -ffp-contract=off --genco -I<repo>/include con_models.hip -o con_models.hsaco
 * tests/test_gpu_batch_constrained.py binds them.
 *
 * Objective: f(x) = sum_i w_i (x_i - c_i)^2, the terms added lane by lane as the header says.
 *   wsq1      ABI 1: c_i = 1 - i / 4, w_i = 1 + i / 2
 *   wsq2      ABI 2: data = c[n] | w[n] (w missing: ones; no data: c = 0)
 *   wsq_rows  ABI 3: the same struct, one data row per search
 * Constraint blocks (value j by ONE lane, sequentially, in the order written):
 *   cubic     m = 1, ABI 2, data = (a, b):  (a x0 + b)^3 - x1
 *   band2     m = 2, ABI 2, data = (lo, hi): lo - x0, x0 - hi
 *   prod3     m = 3, ABI 1:  x_j x_{j+1} - (j + 1) / 2
 *   ball      m = 1, ABI 2, data = (r2):  ((x0^2 + x1^2) + ...) - r2
 *   cuts70    m = 70, ABI 1, n = 8:  ((A_k0 x0 + A_k1 x1) + ...) - b_k,  A_kj = ((7k + 3j) mod 11 - 5) / 8,  b_k = 1 + (k mod 7) / 4
 *   heq2      m = 2, ABI 1 (bound as EQUALITIES):  (x0 + x1) + x2 - 1,  x3 x4 - 1/4 */
#include "nlopt_amd_device.h"

struct Wsq1 {
    static constexpr bool B_IS_PRODUCT = false;
    __device__ static void terms(int n, int i, const double *x, double *a, double *b)
    { const double d = x[i] - (1.0 - 0.25 * i); *a = (1.0 + 0.5 * i) * d * d; *b = 0; }
    __device__ static double finish(int n, double A, double B, const double *x) { return A; }
    __device__ static double grad(int n, int i, const double *x, double A, double B) { return 2 * (1.0 + 0.5 * i) * (x[i] - (1.0 - 0.25 * i)); }
};
NLOPT_AMD_DEVICE_OBJECTIVE(wsq1, Wsq1)

struct Wsq {
    static constexpr bool B_IS_PRODUCT = false;
    __device__ static double c(int n, int i, const void *data, size_t bytes) { return (size_t) (i + 1) * sizeof(double) <= bytes ? ((const double *) data)[i] : 0.; }
    __device__ static double w(int n, int i, const void *data, size_t bytes) { return (size_t) (n + i + 1) * sizeof(double) <= bytes ? ((const double *) data)[n + i] : 1.; }
    __device__ static void terms(int n, int i, const double *x, double *a, double *b, const void *data, size_t bytes)
    { const double d = x[i] - c(n, i, data, bytes); *a = w(n, i, data, bytes) * d * d; *b = 0; }
    __device__ static double finish(int n, double A, double B, const double *x, const void *data, size_t bytes) { return A; }
    __device__ static double grad(int n, int i, const double *x, double A, double B, const void *data, size_t bytes)
    { return 2 * w(n, i, data, bytes) * (x[i] - c(n, i, data, bytes)); }
};
NLOPT_AMD_DEVICE_OBJECTIVE_DATA(wsq2, Wsq)
NLOPT_AMD_DEVICE_OBJECTIVE_ROWS(wsq_rows, Wsq)

struct Cubic {
    __device__ static double value(int n, int j, const double *x, const void *data, size_t bytes)
    {
        const double *p = (const double *) data;
        const double t = p[0] * x[0] + p[1];
        return t * t * t - x[1];
    }
};
NLOPT_AMD_DEVICE_CONSTRAINTS_DATA(cubic, Cubic)

struct Band2 {
    __device__ static double value(int n, int j, const double *x, const void *data, size_t bytes)
    {
        const double *p = (const double *) data;
        return j == 0 ? p[0] - x[0] : x[0] - p[1];
    }
};
NLOPT_AMD_DEVICE_CONSTRAINTS_DATA(band2, Band2)

struct Prod3 {
    __device__ static double value(int n, int j, const double *x) { return x[j] * x[j + 1] - 0.5 * (j + 1); }
};
NLOPT_AMD_DEVICE_CONSTRAINTS(prod3, Prod3)

struct Ball {
    __device__ static double value(int n, int j, const double *x, const void *data, size_t bytes)
    {
        double s = 0;
        for (int i = 0; i < n; ++i) s += x[i] * x[i];
        return s - ((const double *) data)[0];
    }
};
NLOPT_AMD_DEVICE_CONSTRAINTS_DATA(ball, Ball)

struct Cuts70 {
    __device__ static double value(int n, int j, const double *x)
    {
        double s = 0;
        for (int i = 0; i < n; ++i) s += (((7 * j + 3 * i) % 11 - 5) * 0.125) * x[i];
        return s - (1.0 + (j % 7) * 0.25);
    }
};
NLOPT_AMD_DEVICE_CONSTRAINTS(cuts70, Cuts70)

struct Heq2 {
    __device__ static double value(int n, int j, const double *x) { return j == 0 ? x[0] + x[1] + x[2] - 1.0 : x[3] * x[4] - 0.25; }
};
NLOPT_AMD_DEVICE_CONSTRAINTS(heq2, Heq2)
