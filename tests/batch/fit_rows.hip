/* fit_rows.hip — OUT-OF-TREE device objectives for nlopt_amd_optimize_batch, written against include/nlopt_amd_device.h only.
 * Every model is stated ONCE and compiled twice: under the ABI-2 macro (one data block for the optimiser: <name>2, kernel
 * <name>2_evalgrad_d) and under the ABI-3 macro (one data row per search: <name>_rows, kernel <name>_rows_evalgrad_r).  A search on
 * data row k must give the bits of the ABI-2 kernel handed block k alone (tests/test_gpu_batch.py).  Build:
 *     hipcc --offload-arch=gfx950 -O3 -ffp-contract=off --genco -I include tests/batch/fit_rows.hip -o tests/batch/fit_rows.hsaco */
#include <nlopt_amd_device.h>

/* exponential decay: n = 3, x = (a, b, c), block = t[m] | y[m];  r_k = y_k - (a exp(-b t_k) + c) */
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
NLOPT_AMD_DEVICE_RESIDUALS(expfit2, ExpFit, 4)
NLOPT_AMD_DEVICE_RESIDUALS_ROWS(expfit_rows, ExpFit, 4)

/* polynomial fit: block = t[m] | y[m];  r_k = y_k - sum_{i<n} x_i t_k^i, the powers by repeated multiplication */
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
NLOPT_AMD_DEVICE_RESIDUALS(polyfit2, PolyFit<8>, 8)
NLOPT_AMD_DEVICE_RESIDUALS_ROWS(polyfit_rows, PolyFit<8>, 8)

/* the terms / finish / grad form: a sphere whose centre is the block (n doubles) */
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
NLOPT_AMD_DEVICE_OBJECTIVE_DATA(shifted2, Shifted)
NLOPT_AMD_DEVICE_OBJECTIVE_ROWS(shifted_rows, Shifted)
