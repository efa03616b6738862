/* rosen_user.hip — the chained Rosenbrock sum as an OUT-OF-TREE device objective (include/nlopt_amd_device.h), term for term the
 * compiled-in one (csrc/objfuncs.h nla_rosenbrock_term, hip/local_common.h lb_objgrad): tests/test_gpu_tnewton.py compares a search on
 * this kernel — the coroutine, one launch of the user's kernel per evaluation — with the search on the compiled-in objective.  Build:
 *     hipcc --offload-arch=gfx950 -O3 -ffp-contract=off --genco -I include tests/userobj/rosen_user.hip -o tests/userobj/rosen_user.hsaco */
#include <nlopt_amd_device.h>

struct UserRosen {
    static constexpr bool B_IS_PRODUCT = false;
    __device__ static void terms(int n, int i, const double *x, double *a, double *b)
    {
        *a = 0; *b = 0;
        if (i + 1 < n) { const double u = x[i + 1] - x[i] * x[i], v = 1 - x[i]; *a = 100 * (u * u) + v * v; }
    }
    __device__ static double finish(int n, double A, double B, const double *x) { return A; }
    __device__ static double grad(int n, int i, const double *x, double A, double B)
    {
        double gi = 0;
        if (i > 0) { const double a = x[i] - x[i - 1] * x[i - 1]; gi = 200 * a; }
        if (i + 1 < n) { const double a = x[i + 1] - x[i] * x[i], b = 1 - x[i]; gi += -400 * a * x[i] - 2 * b; }
        return gi;
    }
};
NLOPT_AMD_DEVICE_OBJECTIVE(rosen_user, UserRosen)
