/* fit_models.hip — OUT-OF-TREE device objectives and constraints that READ THE CALLER'S DATA, written against
 * include/nlopt_amd_device.h only (ABI 2: NLOPT_AMD_DEVICE_RESIDUALS / _OBJECTIVE_DATA / _CONSTRAINTS_DATA).  Build:
 *     hipcc --offload-arch=gfx950 -O3 -ffp-contract=off --genco -I include tests/userdata/fit_models.hip -o tests/userdata/fit_models.hsaco
 * Bind:  nlopt_amd_set_min_device_objective(opt, ".../fit_models.hsaco", "polyfit", host_twin_or_NULL, twin_data), then
 *        nlopt_amd_set_device_objective_data(opt, t_then_y, 16 * m) */
#include <nlopt_amd_device.h>

/* polynomial fit: data = t[m] | y[m];  r_k = y_k - sum_{i<n} x_i t_k^i  (Horner-free: s = ((x_0 * 1 + x_1 * t) + x_2 * t^2) + ..., the
 * powers by repeated multiplication).  + - * only, so a host twin that restates the order gives the same bits. */
template <int NP>
struct PolyFit {
    __device__ static long count(int n, const void *data, size_t bytes) { return (long) (bytes / (2 * sizeof(double))); }
    template <bool GRAD>
    __device__ static double residual(int n, const double (&x)[NP], long k, const void *data, size_t bytes, double (&d)[NP])
    {
        const long m = (long) (bytes / (2 * sizeof(double)));
        const double *t = (const double *) data, *y = t + m;
        const double tk = t[k];
        double p = 1., s = 0.;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            if (i < n) s += x[i] * p;
            if (GRAD) d[i] = i < n ? -p : 0.;
            p *= tk;
        }
        return y[k] - s;
    }
};
NLOPT_AMD_DEVICE_RESIDUALS(polyfit, PolyFit<8>, 8)
NLOPT_AMD_DEVICE_RESIDUALS(polyfit32, PolyFit<32>, 32)

/* exponential decay: n = 3, x = (a, b, c), data = t[m] | y[m];  r_k = y_k - (a exp(-b t_k) + c) */
struct ExpFit {
    __device__ static long count(int n, const void *data, size_t bytes) { return (long) (bytes / (2 * sizeof(double))); }
    template <bool GRAD>
    __device__ static double residual(int n, const double (&x)[4], long k, const void *data, size_t bytes, double (&d)[4])
    {
        const long m = (long) (bytes / (2 * sizeof(double)));
        const double *t = (const double *) data, *y = t + m;
        const double tk = t[k], e = exp(-x[1] * tk);
        if (GRAD) { d[0] = -e; d[1] = x[0] * tk * e; d[2] = -1.; d[3] = 0.; }
        return y[k] - (x[0] * e + x[2]);
    }
};
NLOPT_AMD_DEVICE_RESIDUALS(expfit, ExpFit, 4)

/* a sphere around a centre taken from the data (n doubles; no data: the origin) — the terms / finish / grad form with data */
struct Shifted {
    static constexpr bool B_IS_PRODUCT = false;
    __device__ static double centre(int i, const void *data, size_t bytes)
    { return (size_t) (i + 1) * sizeof(double) <= bytes ? ((const double *) data)[i] : 0.; }
    __device__ static void terms(int n, int i, const double *x, double *a, double *b, const void *data, size_t bytes)
    { const double v = x[i] - centre(i, data, bytes); *a = v * v; *b = 0; }
    __device__ static double finish(int n, double A, double B, const double *x, const void *data, size_t bytes) { return A; }
    __device__ static double grad(int n, int i, const double *x, double A, double B, const void *data, size_t bytes)
    { return 2 * (x[i] - centre(i, data, bytes)); }
};
NLOPT_AMD_DEVICE_OBJECTIVE_DATA(shifted, Shifted)

/* ... and the same sphere at the origin as an ABI-1 objective: `shifted` with an all-zero centre must give its bits */
struct Sphere1 {
    static constexpr bool B_IS_PRODUCT = false;
    __device__ static void terms(int n, int i, const double *x, double *a, double *b) { *a = x[i] * x[i]; *b = 0; }
    __device__ static double finish(int n, double A, double B, const double *x) { return A; }
    __device__ static double grad(int n, int i, const double *x, double A, double B) { return 2 * x[i]; }
};
NLOPT_AMD_DEVICE_OBJECTIVE(sphere1, Sphere1)

/* linear constraints A x - b <= 0: data = A (m x n, row-major) | b[m];  value j = ((A_j0 x_0 + A_j1 x_1) + ...) - b_j */
struct LinCons {
    __device__ static double value(int n, int j, const double *x, const void *data, size_t bytes)
    {
        const long m = (long) (bytes / sizeof(double)) / (n + 1);
        const double *A = (const double *) data, *b = A + m * n;
        double s = 0;
        for (int i = 0; i < n; ++i) s += A[(long) j * n + i] * x[i];
        return s - b[j];
    }
};
NLOPT_AMD_DEVICE_CONSTRAINTS_DATA(lincons, LinCons)

/* an objective whose <name>_abi reports a version this library does not know: binding it must be refused */
extern "C" __global__ void future_evalgrad_d(int n, int ld, long count, const int *list, const double *X, double *F, double *G, double sign,
                                             const void *data, size_t data_bytes) { }
extern "C" __global__ void future_evalgrad(int n, int ld, long count, const int *list, const double *X, double *F, double *G, double sign) { }
extern "C" __global__ void future_abi(int *out) { *out = 3; }
