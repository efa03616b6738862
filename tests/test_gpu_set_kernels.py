"""-m gpu: the MLSL set launchers (hip/mlsl_kernels.hip) and the three ISRES launchers that draw and evaluate a population
(hip/isres_kernels.hip) against serial statements of their contracts (include/nlopt_amd.h) written here in numpy float64 / Python
— not the product's C code, not oracle/emu_device.c (a second, independent statement: the module also passes over the emulated
device, tools/gpu_suite_on_emu.sh, and that agreement checks the references below).

Launcher                                             test
nla_k_mlsl_rowmin                                    test_rowmin
nla_k_mlsl_colmin                                    test_colmin
nla_k_mlsl_gather_pairs / nla_k_mlsl_gather_pairs_t  test_gather_pairs
nla_k_mlsl_gather_rows                               test_mlsl_gather_rows
nla_k_mlsl_near_bound                                test_near_bound
nla_k_mlsl_negate                                    test_negate
nla_k_isres_nrand                                    test_nrand_*
nla_k_isres_init                                     test_isres_init
nla_k_isres_eval                                     test_isres_eval

Everything here is bit-exact (copied, compared, or computed with IEEE + - * / sqrt only; the tree is built with
-ffp-contract=off) except what passes through device libm: the normal deviates (log) and the objective value, relative 1e-10
(SURVEY.md §7.3.9).  No attempt of the normal-deviate stream is decided by the last bit of s = v1^2 + v2^2: the tests assert
|s - 1| >= 1e-9 over their own inputs before they look at the device, so nothing is excluded from any comparison."""
import ctypes as C
import math

import numpy as np
import pytest

import _oracle as O
import nlopt_amd
from nlopt_amd import DevBuf
from test_gpu_kernels import words_from_seed

pytestmark = pytest.mark.gpu
RTOL = 1e-10
SEED = 2024                       # min |s - 1| over the first 1 053 699 attempts of this stream: 6.5e-7
BORDER = 1e-9
SENT = -7.25
NLA_OBJ_NEGATE = 0x100
vp, i32, i64, f64 = C.c_void_p, C.c_int, C.c_int64, C.c_double
NBIG = (1 << 20) + 5 * 1024 + 3   # 1030 workgroups of 1024 attempts: two tiles of isres_scan_kernel's loop

_cache = {}
MAXDEV = {"z": 0.0}               # largest relative deviation of a deviate seen on the device (printed by every case)


def stream(count):
    if "w" not in _cache or len(_cache["w"]) < count:
        _cache["w"] = words_from_seed(SEED, max(count, 4 * NBIG))
    return _cache["w"][:count].copy()


@pytest.fixture(scope="module")
def L():
    L = nlopt_amd.lib()
    assert nlopt_amd.device_count() > 0, "no HIP device: the product has no CPU fallback"
    L.nla_k_mlsl_rowmin.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, vp]
    L.nla_k_mlsl_colmin.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, vp]
    L.nla_k_mlsl_gather_rows.argtypes = [i32, i32, vp, vp, i32, vp, vp]
    L.nla_k_mlsl_gather_pairs.argtypes = [vp, i32, vp, i32, vp, i32, vp, vp]
    L.nla_k_mlsl_gather_pairs_t.argtypes = [vp, i32, vp, i32, vp, i32, vp, vp]
    L.nla_k_mlsl_near_bound.argtypes = [i32, i32, vp, vp, i32, vp, vp, f64, vp, vp]
    L.nla_k_mlsl_negate.argtypes = [vp, i32, vp]
    L.nla_k_isres_nrand.argtypes = [vp, i64, i64, vp, vp, i64, vp, vp, vp]
    L.nla_k_isres_init.argtypes = [i32, i32, vp, vp, vp, i64, i64, vp, vp, vp, vp]
    L.nla_k_isres_eval.argtypes = [i32, i32, i32, vp, i64, i32, i32, vp, vp, vp, vp, vp, vp]
    for f in (L.nla_k_mlsl_rowmin, L.nla_k_mlsl_colmin, L.nla_k_mlsl_gather_rows, L.nla_k_mlsl_gather_pairs, L.nla_k_mlsl_gather_pairs_t,
              L.nla_k_mlsl_near_bound, L.nla_k_mlsl_negate, L.nla_k_isres_nrand, L.nla_k_isres_init, L.nla_k_isres_eval):
        f.restype = i32
    return L


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def sync(L):
    assert L.nla_stream_sync(None) == 0


# ---- MLSL: minima over qualifying partners (mlsl.c:131-173) ------------------------------------------------------------------
def minima_inputs(na, nb, ldd, variant, seed):
    """D with +inf entries and, beyond column nb, padding that would win every minimum; FA / FB quantised to four levels so that
    equal values are common (a partner with an EQUAL value does not count).  variant "none": no partner qualifies anywhere."""
    rng = np.random.default_rng(seed)
    D = np.full((max(na, 1), ldd), -1.0)
    D[:, :nb] = rng.integers(1, 50, size=(max(na, 1), nb)) / 8.0
    D[:, :nb][rng.random((max(na, 1), nb)) < 0.1] = np.inf
    FA = rng.integers(0, 4, size=max(na, 1)) / 2.0
    FB = rng.integers(0, 4, size=max(nb, 1)) / 2.0
    if variant == "none":
        FA[:] = 1.0
        FB[:] = 1.0
    return D, FA, FB


ROWCOL = [(1, 1, 1), (3, 63, 70), (4, 64, 64), (7, 65, 65), (130, 1000, 1003)]


@pytest.mark.parametrize("na,nb,ldd", ROWCOL + [(5, 0, 4)])
def test_rowmin(L, na, nb, ldd):
    """out[i] = min(init[i], min_j {D[i][j] : FB[j] < FA[i]}), strictly; init NULL = HUGE_VAL"""
    seen_none = seen_some = False
    for variant in ("random", "none", "all"):
        D, FA, FB = minima_inputs(na, nb, ldd, variant, 10 * na + nb)
        if variant == "all":
            FA[:] = 9.0
        elif variant == "random" and na > 1:
            FA[0] = FB[:max(nb, 1)].min()                         # row 0: every partner is equal or larger — none qualifies
        init = np.where(np.arange(na) % 2 == 0, 0.5, np.inf)      # 0.5 beats some of the distances
        dD, dFA, dFB, dinit = DevBuf.from_array(D), DevBuf.from_array(FA), DevBuf.from_array(FB), DevBuf.from_array(init)
        for use_init in (True, False):
            want = np.full(na + 2, SENT)
            for i in range(na):
                cand = D[i, :nb][FB[:nb] < FA[i]]
                m = cand.min() if len(cand) else np.inf
                seen_none |= len(cand) == 0
                seen_some |= len(cand) > 0
                b = init[i] if use_init else np.inf
                want[i] = m if m < b else b
            dout = DevBuf.from_array(np.full(na + 2, SENT))
            assert L.nla_k_mlsl_rowmin(dD.ptr, ldd, na, nb, dFA.ptr, dFB.ptr, dinit.ptr if use_init else None, dout.ptr, None) == 0
            sync(L)
            assert np.array_equal(bits(dout.to_array(np.float64, na + 2)), bits(want)), (variant, use_init)
            dout.free()
    assert seen_none and (seen_some or nb == 0)


@pytest.mark.parametrize("na,nb,ldd", ROWCOL)
def test_colmin(L, na, nb, ldd):
    """inout[j] = min(inout[j], min_i {D[i][j] : FA[i] < FB[j]}) where skip[j] == 0 (skip NULL: everywhere); a skipped column
    keeps its value even when a smaller distance qualifies; na = 0 changes nothing"""
    rng = np.random.default_rng(7 * na + nb)
    for variant in ("random", "none", "all"):
        D, FA, FB = minima_inputs(na, nb, ldd, variant, 20 * na + nb)
        if variant == "all":
            FB[:] = 9.0
        elif variant == "random" and nb > 1:
            FB[0] = FA.min()                                      # column 0: no partner qualifies
        inout0 = np.full(nb + 2, SENT)
        inout0[:nb] = np.where(rng.random(nb) < 0.3, 0.25, 1e9)  # 0.25: smaller than some of the column's distances
        skip = (rng.random(nb) < 0.4).astype(np.int32)
        if variant == "all":
            skip[0] = 1
            inout0[0] = 1e9                                       # a smaller distance exists and qualifies: must stay
        dD, dFA, dFB, dskip = DevBuf.from_array(D), DevBuf.from_array(FA), DevBuf.from_array(FB), DevBuf.from_array(skip)
        for use_skip in (True, False):
            for rows in (na, 0):
                want = inout0.copy()
                for j in range(nb):
                    if use_skip and skip[j]:
                        continue
                    cand = D[:rows, j][FA[:rows] < FB[j]]
                    if len(cand) and cand.min() < want[j]:
                        want[j] = cand.min()
                dio = DevBuf.from_array(inout0)
                assert L.nla_k_mlsl_colmin(dD.ptr, ldd, rows, nb, dFA.ptr, dFB.ptr, dskip.ptr if use_skip else None, dio.ptr, None) == 0
                sync(L)
                assert np.array_equal(bits(dio.to_array(np.float64, nb + 2)), bits(want)), (variant, use_skip, rows)
                if rows == 0:
                    assert np.array_equal(want, inout0)
                dio.free()
        if variant == "all":
            assert D[:na, 0].min() < 1e9


@pytest.mark.parametrize("nc", [1, 255, 256, 257])
@pytest.mark.parametrize("nr", [1, 3])
def test_gather_pairs(L, nr, nc):
    """out[a nc + b] (transposed: out[b nr + a]) = D[rows[a] ldd + cols[b]], repeated indices, ldd beyond the largest column"""
    rng = np.random.default_rng(1000 * nr + nc)
    nrowsD, ncolsD, ldd = 9, 300, 307
    D = rng.uniform(0, 10, size=(nrowsD, ldd))
    D[2, 5] = -0.0
    rows = rng.integers(0, nrowsD, size=nr).astype(np.int64)
    cols = rng.integers(0, ncolsD, size=nc).astype(np.int64)
    if nr > 1:
        rows[1] = rows[0]
    if nc > 1:
        cols[1], cols[nc - 1] = cols[0], ncolsD - 1
    sub = D[rows][:, cols]
    dD, dr, dc = DevBuf.from_array(D), DevBuf.from_array(rows), DevBuf.from_array(cols)
    for fn, want in ((L.nla_k_mlsl_gather_pairs, sub), (L.nla_k_mlsl_gather_pairs_t, sub.T)):
        dout = DevBuf.from_array(np.full(nr * nc + 3, SENT))
        assert fn(dD.ptr, ldd, dr.ptr, nr, dc.ptr, nc, dout.ptr, None) == 0
        sync(L)
        got = dout.to_array(np.float64, nr * nc + 3)
        assert np.array_equal(bits(got[:nr * nc]), bits(want).ravel()) and np.all(got[nr * nc:] == SENT)
        dout.free()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_mlsl_gather_rows(L, n):
    """dst row c := src row idx[c]: repeated indices, destination padding untouched"""
    rng = np.random.default_rng(n)
    ld, nsrc = n + 2, 11
    src = rng.uniform(-3, 3, size=(nsrc, ld))
    src[4, 0] = -0.0
    dsrc = DevBuf.from_array(src)
    for count in (1, 3):
        idx = np.array([4, 9, 4][:count], np.int64)
        dst0 = np.full((count + 1, ld), SENT)
        want = dst0.copy()
        want[:count, :n] = src[idx, :n]
        didx, ddst = DevBuf.from_array(idx), DevBuf.from_array(dst0)
        assert L.nla_k_mlsl_gather_rows(n, ld, dsrc.ptr, didx.ptr, count, ddst.ptr, None) == 0
        sync(L)
        assert np.array_equal(bits(ddst.to_array(np.float64, (count + 1) * ld)), bits(want).ravel())
        ddst.free()


@pytest.mark.parametrize("n", [1, 300, 600])
def test_near_bound(L, n):
    """flags[c] = some coordinate j of row idx[c] has (x - lb <= thr or ub - x <= thr) and ub - lb > thr (mlsl.c:211-218).
    Dyadic numbers throughout: the comparisons at equality are exact.  Box A: every side 8 wide.  Box B: as A, but the side of
    one coordinate is exactly thr wide — every x is "near" there, and it must not count."""
    thr, eps = 0.5, 2.0 ** -40
    ld = n + 1
    lbA, ubA = np.full(n, -2.0), np.full(n, 6.0)
    jn = n // 2
    lbB, ubB = lbA.copy(), ubA.copy()
    ubB[jn] = lbB[jn] + thr
    mid = np.full(n, 2.0)
    rows, wantA = [], []

    def add(j, x, hit):
        r = mid.copy()
        if j is not None:
            r[j] = x
        rows.append(r)
        wantA.append(hit)

    add(None, 0, 0)                                       # nothing near a bound
    add(0, -2.0 + thr, 1)                                 # x - lb == thr: a hit
    add(0, 6.0 - thr, 1)                                  # ub - x == thr: a hit
    add(0, -2.0 + thr + eps, 0)                           # just beyond either: none
    add(0, 6.0 - thr - eps, 0)
    add(n - 1, 6.0, 1)                                    # the only hit at the last coordinate
    if n > 256:
        add(256, -2.0, 1)                                 # ... in the second pass of the thread stride
        add(n - 2, 6.0 - thr, 1)
    P = np.full((len(rows), ld), -2.0)                    # padding: would be a hit if it were read as a coordinate
    P[:, :n] = np.array(rows)
    wantA = np.array(wantA, np.int32)
    # box B: coordinate jn sits in its thr-wide side (x = lb + thr / 2: near both bounds) in every row
    PB = P.copy()
    PB[:, jn] = lbB[jn] + thr / 2
    wantB = wantA.copy()
    hitcoord = [None, 0, 0, None, None, n - 1] + ([256, n - 2] if n > 256 else [])
    for r, j in enumerate(hitcoord):
        if j == jn:
            wantB[r] = 0                                  # the row's only hit was moved into the narrow side
    idx = np.array(list(range(len(rows))) + [1, 0, 1], np.int64)[::-1].copy()
    for Pm, lb, ub, want in ((P, lbA, ubA, wantA), (PB, lbB, ubB, wantB)):
        ref = np.array([int(any((x[j] - lb[j] <= thr or ub[j] - x[j] <= thr) and ub[j] - lb[j] > thr for j in range(n))) for x in Pm], np.int32)
        assert np.array_equal(ref, want)                  # the table above is what the contract says
        dP, dlb, dub, didx = DevBuf.from_array(Pm), DevBuf.from_array(lb), DevBuf.from_array(ub), DevBuf.from_array(idx)
        dfl = DevBuf.from_array(np.full(len(idx) + 1, -9, np.int32))
        assert L.nla_k_mlsl_near_bound(n, ld, dP.ptr, didx.ptr, len(idx), dlb.ptr, dub.ptr, thr, dfl.ptr, None) == 0
        sync(L)
        got = dfl.to_array(np.int32, len(idx) + 1)
        assert np.array_equal(got[:-1], want[idx]) and got[-1] == -9
    assert wantB[0] == 0 and (n == 1 or wantB[1] == 1)    # box B: the narrow side alone is no hit; a real hit beside it still is


@pytest.mark.parametrize("count", [1, 255, 256, 257])
def test_negate(L, count):
    rng = np.random.default_rng(count)
    F = np.full(count + 1, SENT)
    F[:count] = rng.uniform(-5, 5, size=count)
    special = np.array([0.0, -0.0, np.inf, -np.inf, 5e-324])
    k = np.arange(count)
    F[:count] = np.where(k % 3 == 0, special[k % 5], F[:count])
    want = F.copy()
    want[:count] = -F[:count]
    assert np.signbit(want[0]) and want[0] == 0.0         # +0.0 became -0.0
    dF = DevBuf.from_array(F)
    assert L.nla_k_mlsl_negate(dF.ptr, count, None) == 0
    sync(L)
    assert np.array_equal(bits(dF.to_array(np.float64, count + 1)), bits(want))


# ---- ISRES: normal deviates (mt19937ar.c:216-232) ---------------------------------------------------------------------------
def urand(a, b, w):
    w = w.astype(np.uint64)
    u = ((w[0::2] >> np.uint64(5)) * 67108864.0 + (w[1::2] >> np.uint64(6)).astype(np.float64)) * (1.0 / 9007199254740992.0)
    return a + (b - a) * u


def nrand_attempts(w):
    """every 4-word attempt of w: accepted? and the deviate"""
    v = urand(-1.0, 1.0, w)
    v1, v2 = v[0::2], v[1::2]
    s = v1 * v1 + v2 * v2
    assert np.abs(s - 1.0).min() >= BORDER, "an attempt of this stream is decided by the last bit of s"
    ok = ~(s >= 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(s == 0, 0.0, v1 * np.sqrt(-2 * np.log(s) / s))
    return ok, z


class Nrand:
    def __init__(self, cap):
        self.cap = cap
        self.z = DevBuf.from_array(np.full(cap, SENT))
        self.zatt = DevBuf.from_array(np.full(cap, -12345, np.int64))
        self.ztotal = DevBuf.from_array(np.zeros(1, np.int64))

    def launch(self, L, w, nattempts, attempt_base, zbase):
        dw = DevBuf.from_array(w)
        counts = DevBuf(4 * ((nattempts + 1023) // 1024))
        assert L.nla_k_isres_nrand(dw.ptr, nattempts, attempt_base, counts.ptr, self.ztotal.ptr, zbase, self.z.ptr, self.zatt.ptr, None) == 0
        sync(L)
        dw.free()
        counts.free()

    def read(self):
        return self.z.to_array(np.float64, self.cap), self.zatt.to_array(np.int64, self.cap), int(self.ztotal.to_array(np.int64, 1)[0])


def check_nrand(got, ok, zref):
    z, zatt, ztotal = got
    idx = np.flatnonzero(ok)
    k = len(idx)
    assert ztotal == k
    assert np.array_equal(zatt[:k], idx)
    want = zref[idx]
    nz = want != 0
    if nz.any():
        MAXDEV["z"] = max(MAXDEV["z"], float((np.abs(z[:k][nz] - want[nz]) / np.abs(want[nz])).max()))
    print("largest relative deviation of z so far: %.3g" % MAXDEV["z"])
    assert np.all(np.abs(z[:k] - want) <= RTOL * np.abs(want))
    assert np.all(z[k:] == SENT) and np.all(zatt[k:] == -12345)


@pytest.mark.parametrize("nattempts", [1, 1023, 1025, NBIG])
def test_nrand_compaction_equals_the_masked_reference(L, nattempts):
    w = stream(4 * nattempts)
    ok, zref = nrand_attempts(w)
    t = Nrand(int(ok.sum()) + 64)
    t.launch(L, w, nattempts, 0, 0)
    check_nrand(t.read(), ok, zref)


def test_nrand_second_launch_appends(L):
    n1, n2 = 5000, 7001
    w = stream(4 * (n1 + n2))
    ok, zref = nrand_attempts(w)
    t = Nrand(int(ok.sum()) + 64)
    t.launch(L, w[:4 * n1], n1, 0, 0)
    first = t.read()
    assert first[2] == int(ok[:n1].sum())
    t.launch(L, w[4 * n1:], n2, n1, first[2])
    check_nrand(t.read(), ok, zref)
    one = Nrand(int(ok.sum()) + 64)
    one.launch(L, w, n1 + n2, 0, 0)
    a, b = t.read(), one.read()
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]) and a[2] == b[2]


# ---- ISRES: initial population (isres.c:122-128) ------------------------------------------------------------------------------
@pytest.mark.parametrize("n,ld", [(1, 2), (63, 64), (64, 64), (65, 66), (130, 130), (65, 72)])
def test_isres_init(L, n, ld):
    """individuals k_first .. k_first + count - 1: X[k][j] = lb_j + (ub_j - lb_j) u from the individual's own words, individual 0
    := x0 bit for bit; S = (ub - lb) / sqrt(n); other rows and the padding untouched"""
    rng = np.random.default_rng(n + ld)
    lb, ub = np.linspace(-3.0, -0.5, n), np.linspace(0.25, 11.0, n)
    x0 = rng.uniform(-0.5, 0.25, size=n)
    x0[0] = -0.0
    dlb, dub, dx0 = DevBuf.from_array(lb), DevBuf.from_array(ub), DevBuf.from_array(x0)
    for count in (1, 5, 9):
        w = stream(2 * n * 9 + 4)[4:4 + 2 * n * count]
        for k_first in (0, 5):
            rows = k_first + count + 1
            X0 = np.full((rows, ld), SENT)
            wantX, wantS = X0.copy(), X0.copy()
            for kl in range(count):
                k = k_first + kl
                wantX[k, :n] = x0 if k == 0 else urand(lb, ub, w[2 * n * kl:2 * n * (kl + 1)])
                wantS[k, :n] = (ub - lb) / np.sqrt(float(n))
            dw, dX, dS = DevBuf.from_array(w), DevBuf.from_array(X0), DevBuf.from_array(X0)
            assert L.nla_k_isres_init(n, ld, dlb.ptr, dub.ptr, dw.ptr, k_first, count, dx0.ptr, dX.ptr, dS.ptr, None) == 0
            sync(L)
            X, S = dX.to_array(np.float64, rows * ld).reshape(rows, ld), dS.to_array(np.float64, rows * ld).reshape(rows, ld)
            assert np.array_equal(bits(X), bits(wantX)), (count, k_first)
            assert np.array_equal(bits(S), bits(wantS)), (count, k_first)
            if k_first:
                assert not np.array_equal(X[k_first, :n], x0) and np.all(X[:k_first] == SENT)
            for d in (dw, dX, dS):
                d.free()


# ---- ISRES: f and the penalties (isres.c:138-166) ------------------------------------------------------------------------------
CON = np.dtype([("type", "<i4"), ("q", "<u4"), ("Q", "<u4"), ("pad", "<i4"), ("tol", "<f8")])      # nla_dev_constraint
EVAL_N, EVAL_POP = 130, 9
TOLS = (0.0, 0.125, 0.5)


def eval_inputs(m, p):
    """block-sum constraints g = sum_{i in block q of Q} x_i - 1, Q = min(n, m + p), tolerances 0 / 1/8 / 1/2 in turn.  Rows:
    0: zeros (every g = -1); 1: every g equals its tolerance exactly; 2: every g exceeds it by 1/4; 3-5: multiples of 1/64;
    6-8: arbitrary doubles (the order of the sums shows)."""
    n, mp = EVAL_N, m + p
    rng = np.random.default_rng(50 * m + p)
    con = np.zeros(max(mp, 1), CON)
    Q = max(1, min(n, mp))
    for c in range(mp):
        con[c] = (0, c % Q, Q, 0, TOLS[(c % Q) % 3])
    X = np.zeros((EVAL_POP, n))
    for c in range(min(mp, Q)):
        lo = (c * n) // Q
        X[1, lo] = 1.0 + TOLS[c % 3]
        X[2, lo] = 1.25 + TOLS[c % 3]
    X[3:6] = rng.integers(-128, 129, size=(3, n)) / 64.0
    X[6:9] = rng.uniform(-1.5, 1.5, size=(3, n))
    return con, X


def eval_reference(X, m, p, con):
    n = X.shape[1]
    F, PEN, GPEN, FEAS = [], [], [], []
    seen = set()
    for x in X.tolist():
        pen = gpen = 0.0
        feas = 1
        for c in range(m + p):
            q, Q, tol = int(con[c]["q"]), int(con[c]["Q"]), float(con[c]["tol"])
            s = 0.0
            for i in range((q * n) // Q, ((q + 1) * n) // Q):
                s += x[i]
            g = s - 1.0
            seen.add("neg" if g < 0 else "eq" if g == tol else "over" if g > tol else "under")
            if c == m:
                gpen = pen
            if c < m:
                if g > tol:
                    feas = 0
                if g < 0:
                    g = 0.0
                pen += g * g
            else:
                if abs(g) > tol:
                    feas = 0
                pen += g * g
        if p == 0:
            gpen = pen
        F.append(math.fsum(v * v for v in x))
        PEN.append(pen)
        GPEN.append(gpen)
        FEAS.append(feas)
    return np.array(F), np.array(PEN), np.array(GPEN), np.array(FEAS, np.int32), seen


def run_eval(L, obj, X, m, p, con):
    pop, n = X.shape
    dX, dcon = DevBuf.from_array(X), DevBuf.from_array(con)
    dF, dP, dG = (DevBuf.from_array(np.full(pop + 1, SENT)) for _ in range(3))
    dfe = DevBuf.from_array(np.full(pop + 1, -9, np.int32))
    assert L.nla_k_isres_eval(obj, n, n, dX.ptr, pop, m, p, dcon.ptr, dF.ptr, dP.ptr, dG.ptr, dfe.ptr, None) == 0
    sync(L)
    F, PEN, GPEN = (d.to_array(np.float64, pop + 1) for d in (dF, dP, dG))
    FEAS = dfe.to_array(np.int32, pop + 1)
    assert F[pop] == SENT and PEN[pop] == SENT and GPEN[pop] == SENT and FEAS[pop] == -9
    return F[:pop], PEN[:pop], GPEN[:pop], FEAS[:pop]


@pytest.mark.parametrize("m,p", [(0, 0), (1, 0), (0, 1), (4, 3), (63, 2), (64, 0), (64, 1), (65, 70), (0, 130)])
def test_isres_eval(L, m, p):
    """PEN = sum max(g, 0)^2 + sum h^2 in constraint order, GPEN = its value before the first equality (= PEN when p = 0), FEAS =
    every g <= tol and |h| <= tol: exact, across the 64-constraint tiles of the kernel (m on and beside a tile edge); F within
    1e-10 of math.fsum"""
    sphere = O.OBJ["sphere"]
    con, X = eval_inputs(m, p)
    Fr, PENr, GPENr, FEASr, seen = eval_reference(X, m, p, con)
    assert m + p == 0 or {"neg", "eq", "over"} <= seen
    assert m + p == 0 or (FEASr[1] == 1 and FEASr[2] == 0)
    F, PEN, GPEN, FEAS = run_eval(L, sphere, X, m, p, con)
    assert np.array_equal(bits(PEN), bits(PENr)) and np.array_equal(bits(GPEN), bits(GPENr)) and np.array_equal(FEAS, FEASr)
    assert np.all(np.abs(F - Fr) <= RTOL * np.abs(Fr))
    if (m, p) in ((4, 3), (65, 70)):
        # obj < 0: the constraint part only, F untouched
        F2, PEN2, GPEN2, FEAS2 = run_eval(L, -1, X, m, p, con)
        assert np.all(F2 == SENT)
        assert np.array_equal(bits(PEN2), bits(PENr)) and np.array_equal(bits(GPEN2), bits(GPENr)) and np.array_equal(FEAS2, FEASr)
        # NLA_OBJ_NEGATE: F = -f
        F3, PEN3, _, _ = run_eval(L, sphere | NLA_OBJ_NEGATE, X, m, p, con)
        assert np.array_equal(bits(F3), bits(-F)) and np.array_equal(bits(PEN3), bits(PENr))
