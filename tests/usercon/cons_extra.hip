// cons_extra.hip — example user-supplied device constraints for libnlopt_amd (NLOPT_GN_ISRES), written against
// include/nlopt_amd_device.h only.  Build:
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off --genco -I<repo>/include cons_extra.hip -o cons_extra.hsaco
// Every value uses + - * only, in one fixed order, so a host twin written as the same sequential loops gives the same bits.
#include "nlopt_amd_device.h"

#define CONS_R 60.0
#define CONS_C 1.0
#define CONS_D 1.5

__device__ static double g0(int n, const double *x) { double s = 0; for (int i = 0; i < n; ++i) s += x[i] * x[i]; return s - CONS_R; }
__device__ static double g1(int n, const double *x) { return x[0] * x[n > 1 ? 1 : 0] - CONS_C; }
__device__ static double g2(int n, const double *x) { double s = 0; for (int i = 1; i < n; i += 2) s += x[i]; return s - 1.0; }
__device__ static double h0(int n, const double *x) { return x[0] + 2.0 * x[n - 1] - CONS_D; }

// cons: g0, g1, g2, h0 (bind with m <= 4: the first m of them)
struct Cons {
    __device__ static double value(int n, int j, const double *x) { return j == 0 ? g0(n, x) : j == 1 ? g1(n, x) : j == 2 ? g2(n, x) : h0(n, x); }
};
NLOPT_AMD_DEVICE_CONSTRAINTS(cons, Cons)

// pair: g0, g2
struct Pair {
    __device__ static double value(int n, int j, const double *x) { return j == 0 ? g0(n, x) : g2(n, x); }
};
NLOPT_AMD_DEVICE_CONSTRAINTS(pair, Pair)

// eqh: h0
struct EqH {
    __device__ static double value(int n, int, const double *x) { return h0(n, x); }
};
NLOPT_AMD_DEVICE_CONSTRAINTS(eqh, EqH)

// many: g_j = x_{j mod n} (j + 1) - 1, as many as asked for (the tests bind 70: more than one 64-entry chunk of the fold)
struct Many {
    __device__ static double value(int n, int j, const double *x) { return x[j % n] * (double) (j + 1) - 1.0; }
};
NLOPT_AMD_DEVICE_CONSTRAINTS(many, Many)

// an objective under the SAME name as the block `cons` (cons_evalgrad / cons_abi beside cons_coneval / cons_conabi): f = sum (x_i - 0.3)^2,
// summed sequentially inside finish(), which every lane runs on the whole x — no reduction across lanes takes part, so f too equals a
// sequential host twin bit for bit and a run on the device equals the host-callback run exactly
struct SeqSphere {
    static constexpr bool B_IS_PRODUCT = false;
    __device__ static void terms(int, int, const double *, double *a, double *b) { *a = 0; *b = 0; }
    __device__ static double finish(int n, double, double, const double *x)
    { double s = 0; for (int i = 0; i < n; ++i) { const double d = x[i] - 0.3; s += d * d; } return s; }
    __device__ static double grad(int, int i, const double *x, double, double) { return 2.0 * (x[i] - 0.3); }
};
NLOPT_AMD_DEVICE_OBJECTIVE(cons, SeqSphere)
