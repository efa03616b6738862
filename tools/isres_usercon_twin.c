/* isres_usercon_twin.c — host twins of the first three constraints of tests/usercon/cons_extra.hip (g0, g1, g2) as one nlopt_mfunc,
 * for tools/isres_usercon_bench.py: the same sequential formulas, compiled with -ffp-contract=off.  What a user of
 * nlopt_add_inequality_mconstraint would write in C. */
void cons_twin(unsigned m, double *result, unsigned n, const double *x, double *grad, void *data)
{
    unsigned i, j;
    (void) grad; (void) data;
    for (j = 0; j < m; ++j) {
        double s = 0;
        if (j == 0) { for (i = 0; i < n; ++i) s += x[i] * x[i]; result[j] = s - 60.0; }
        else if (j == 1) result[j] = x[0] * x[n > 1 ? 1 : 0] - 1.0;
        else { for (i = 1; i < n; i += 2) s += x[i]; result[j] = s - 1.0; }
    }
}
