/* userdata_fit_twin.c — the sample `expfit` of tests/userdata/fit_models.hip as an ordinary C nlopt_func, for tools/userdata_fit_bench.py:
 * f(a, b, c) = sum_k (y_k - (a exp(-b t_k) + c))^2 over the m data points behind f_data, summed sequentially — the way such an
 * objective had to be written before device objectives could read data (one point per call, on the caller's thread). */
#include <math.h>

typedef struct { long m; const double *t, *y; } fit_data;

double expfit_twin(unsigned n, const double *x, double *grad, void *data)
{
    const fit_data *d = (const fit_data *) data;
    double f = 0, g0 = 0, g1 = 0, g2 = 0;
    long k;
    (void) n;
    for (k = 0; k < d->m; ++k) {
        const double e = exp(-x[1] * d->t[k]), r = d->y[k] - (x[0] * e + x[2]);
        f += r * r;
        if (grad) { g0 += r * -e; g1 += r * (x[0] * d->t[k] * e); g2 -= r; }
    }
    if (grad) { grad[0] = 2 * g0; grad[1] = 2 * g1; grad[2] = 2 * g2; }
    return f;
}
