"""-m gpu: every ESCH launcher of include/nlopt_amd.h (hip/esch_kernels.hip) against a serial statement of its contract written
here in numpy float64 / Python — not the product's C code, not oracle/emu_device.c (which is a second, independent statement: the
module also passes over the emulated device, tools/gpu_suite_on_emu.sh, and that agreement checks the references below).

Launcher                      test
nla_k_esch_cauchy             test_cauchy_*            (1 / 1023 / 1024 / 1025 attempts, 1028 workgroups = two counts per scan
                                                        thread, an appending second launch, vcap inside a workgroup)
nla_k_esch_fill_rows          test_fill_rows
nla_k_esch_crossover          test_crossover
nla_k_esch_gather_rows        test_gather_rows
nla_k_esch_select             test_select_is_a_stable_sort
nla_k_esch_mutate             test_mutate_*            (driver-sized segments, contention, > 128 blocks, exact fit, too short and
                                                        retried, crafted straddles of block and tile edges)
nla_esch_mut_scratch_bytes / nla_esch_sort_scratch_bytes size every scratch buffer.

Bit-exact: integer / index / count outputs, everything copied or selected, everything computed with IEEE + - * / only (the tree
is built with -ffp-contract=off).  Relative 1e-10 (device libm against glibc): what passes through tan().
No random-word case contains an attempt whose accept / reject decision could depend on the last bit of tan(): every test asserts
||c| - 5| >= 1e-9 over its own inputs before it looks at the device, so nothing is excluded from any comparison."""
import ctypes as C

import numpy as np
import pytest

import nlopt_amd
from nlopt_amd import DevBuf
from test_gpu_kernels import words_from_seed

pytestmark = pytest.mark.gpu
RTOL = 1e-10
SEED = 2024                       # min ||c| - 5| over the first 1 051 665 attempts of this stream: 3.4e-6
BORDER = 1e-9
BLOCK = 4096                      # stream words per block of the mutation chain (ESCH_BLOCK)
SENT = -7.25                      # never a value of v (in [0, 1]) or of a row
vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
NBIG = (1 << 20) + 3 * 1024 + 17  # 1028 workgroups of 1024 attempts: esch_scan_kernel's threads take two counts each

_cache = {}
MAXDEV = {"v": 0.0}               # largest relative deviation of an accepted value seen on the device (printed by every case)


def stream(count):
    """the first `count` words of the reference's MT19937 stream for SEED (generated once)"""
    if "w" not in _cache or len(_cache["w"]) < count:
        _cache["w"] = words_from_seed(SEED, max(count, 2 * NBIG))
    return _cache["w"][:count].copy()


@pytest.fixture(scope="module")
def L():
    L = nlopt_amd.lib()
    assert nlopt_amd.device_count() > 0, "no HIP device: the product has no CPU fallback"
    L.nla_k_esch_cauchy.argtypes = [vp, i64, i64, vp, vp, i64, i64, vp, vp, vp]
    L.nla_k_esch_fill_rows.argtypes = [i32, i32, vp, vp, vp, i64, i64, vp, vp]
    L.nla_k_esch_crossover.argtypes = [i32, i32, i64, i64, vp, vp, vp, vp]
    L.nla_esch_mut_scratch_bytes.argtypes = [i64]
    L.nla_esch_mut_scratch_bytes.restype = C.c_size_t
    L.nla_k_esch_mutate.argtypes = [vp, i64, i64, i32, i32, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp]
    L.nla_k_esch_gather_rows.argtypes = [i32, i32, vp, i64, i64, vp, vp, vp]
    L.nla_esch_sort_scratch_bytes.argtypes = [i64]
    L.nla_esch_sort_scratch_bytes.restype = C.c_size_t
    L.nla_k_esch_select.argtypes = [i64, vp, vp, vp, vp, vp, C.c_size_t, vp]
    for f in (L.nla_k_esch_cauchy, L.nla_k_esch_fill_rows, L.nla_k_esch_crossover, L.nla_k_esch_mutate, L.nla_k_esch_gather_rows,
              L.nla_k_esch_select):
        f.restype = i32
    return L


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- the serial statement of randcauchy (esch.c:28-50) ----------------------------------------------------------------
def u_of(w):
    """nlopt_urand(0, 1) of consecutive word pairs: 53-bit resolution, a + (b - a) u with a = 0, b = 1"""
    w = w.astype(np.uint64)
    return ((w[0::2] >> np.uint64(5)) * 67108864.0 + (w[1::2] >> np.uint64(6)).astype(np.float64)) * (1.0 / 9007199254740992.0)


def cauchy_attempts(w, random_words=True):
    """every 2-word attempt of w: accepted? and the value folded to [0, 1]"""
    c = np.tan((u_of(w) - 0.5) * np.pi)
    if random_words and len(c):
        assert np.abs(np.abs(c) - 5.0).min() >= BORDER, "an attempt of this stream is decided by the last bit of tan()"
    ok = ~((c < -5.0) | (c > 5.0))
    return ok, np.where(c < 0, -c, c + 5.0) / 10.0


def note_dev(got, want):
    nz = want != 0
    if nz.any():
        MAXDEV["v"] = max(MAXDEV["v"], float((np.abs(got[nz] - want[nz]) / np.abs(want[nz])).max()))
    print("largest relative deviation of v so far: %.3g" % MAXDEV["v"])
    assert np.all(np.abs(got - want) <= RTOL * np.abs(want))


class Cauchy:
    """device buffers of one compaction target: v / vatt of `cap` entries behind sentinels, the vtotal cell"""

    def __init__(self, cap):
        self.cap = cap
        self.v = DevBuf.from_array(np.full(cap, SENT))
        self.vatt = DevBuf.from_array(np.full(cap, -12345, np.int64))
        self.vtotal = DevBuf.from_array(np.zeros(1, np.int64))

    def launch(self, L, w, nattempts, attempt_base, vbase, vcap):
        dw = DevBuf.from_array(w)
        counts = DevBuf(4 * ((nattempts + 1023) // 1024))
        assert L.nla_k_esch_cauchy(dw.ptr, nattempts, attempt_base, counts.ptr, self.vtotal.ptr, vbase, vcap, self.v.ptr, self.vatt.ptr, None) == 0
        assert L.nla_stream_sync(None) == 0
        dw.free()
        counts.free()

    def read(self):
        return self.v.to_array(np.float64, self.cap), self.vatt.to_array(np.int64, self.cap), int(self.vtotal.to_array(np.int64, 1)[0])


def check_cauchy(got, ok, val, written):
    """v / vatt hold the accepted attempts in order in [0, written), sentinels behind; vtotal counts every accepted attempt"""
    v, vatt, vtotal = got
    idx = np.flatnonzero(ok)
    assert vtotal == len(idx)
    assert np.array_equal(vatt[:written], idx[:written])
    note_dev(v[:written], val[idx[:written]])
    assert np.all(v[written:] == SENT) and np.all(vatt[written:] == -12345)


@pytest.mark.parametrize("nattempts", [1, 1023, 1024, 1025, NBIG])
def test_cauchy_compaction_equals_the_masked_reference(L, nattempts):
    w = stream(2 * nattempts)
    ok, val = cauchy_attempts(w)
    nacc = int(ok.sum())
    t = Cauchy(nacc + 64)
    t.launch(L, w, nattempts, 0, 0, nacc + 64)
    check_cauchy(t.read(), ok, val, nacc)


def test_cauchy_second_launch_appends(L):
    """attempts [0, 5000) then [5000, 12001) with attempt_base, vbase and the same vtotal cell == one launch over 12 001"""
    n1, n2 = 5000, 7001
    w = stream(2 * (n1 + n2))
    ok, val = cauchy_attempts(w)
    nacc, nacc1 = int(ok.sum()), int(ok[:n1].sum())
    t = Cauchy(nacc + 64)
    t.launch(L, w[:2 * n1], n1, 0, 0, nacc + 64)
    first = t.read()
    assert first[2] == nacc1
    t.launch(L, w[2 * n1:], n2, n1, first[2], nacc + 64)
    check_cauchy(t.read(), ok, val, nacc)
    one = Cauchy(nacc + 64)
    one.launch(L, w, n1 + n2, 0, 0, nacc + 64)
    a, b = t.read(), one.read()
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def test_cauchy_vcap_inside_a_workgroup(L):
    """vcap = vbase + 1500 falls among the values of the second of four workgroups: nothing at or beyond it is written, and
    *vtotal still counts every accepted attempt"""
    nattempts, vbase = 4096, 37
    w = stream(2 * nattempts)
    ok, val = cauchy_attempts(w)
    idx = np.flatnonzero(ok)
    assert int(ok[:1024].sum()) < 1500 < int(ok[:2048].sum())
    t = Cauchy(vbase + len(idx) + 64)
    t.launch(L, w, nattempts, 0, vbase, vbase + 1500)
    v, vatt, vtotal = t.read()
    assert vtotal == len(idx)
    assert np.all(v[:vbase] == SENT) and np.all(vatt[:vbase] == -12345)
    assert np.array_equal(vatt[vbase:vbase + 1500], idx[:1500])
    note_dev(v[vbase:vbase + 1500], val[idx[:1500]])
    assert np.all(v[vbase + 1500:] == SENT) and np.all(vatt[vbase + 1500:] == -12345)


# ---- rows ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,ld", [(1, 2), (5, 6), (257, 258), (600, 600)])
def test_fill_rows(L, n, ld):
    """element e = id n + item := lb + (ub - lb) v[e - e0] for e in [e0, e0 + count), e0 inside a row (n = 1 has no inside);
    rows, elements and padding outside the range keep their bits"""
    rng = np.random.default_rng(n)
    lb, ub = np.linspace(-3.0, -1.0, n), np.linspace(0.5, 7.0, n)
    e0 = 3 if n == 1 else 2 * n + n // 2 + 1
    assert n == 1 or e0 % n
    dlb, dub = DevBuf.from_array(lb), DevBuf.from_array(ub)
    for count in (1, 255, 256, 257, 3 * n + 1):
        rows = (e0 + count) // n + 2
        v = rng.random(count)
        R0 = np.full((rows, ld), SENT)
        want = R0.copy()
        e = e0 + np.arange(count)
        want[e // n, e % n] = lb[e % n] + (ub[e % n] - lb[e % n]) * v
        dv, dR = DevBuf.from_array(v), DevBuf.from_array(R0)
        assert L.nla_k_esch_fill_rows(n, ld, dlb.ptr, dub.ptr, dv.ptr, e0, count, dR.ptr, None) == 0
        assert L.nla_stream_sync(None) == 0
        assert np.array_equal(bits(dR.to_array(np.float64, rows * ld)), bits(want).ravel()), count
        dv.free()
        dR.free()


@pytest.mark.parametrize("n,npar,no", [(1, 3, 5), (2, 7, 7), (257, 40, 60), (600, 3, 130)])
def test_crossover(L, n, npar, no):
    """offspring id := parent p1's items below `cross`, parent p2's from there on (esch.c:192-203), rows through a slot table
    that is a random permutation; cross = 0, cross = n - 1 and p1 == p2 forced in the first three offspring"""
    rng = np.random.default_rng(100 + n)
    ld = n + 3
    w = rng.integers(0, 1 << 32, size=3 * no, dtype=np.uint64).astype(np.uint32)
    w[2] = 5 * n                                    # cross = 0
    w[5] = 7 * n + n - 1                            # cross = n - 1
    w[6] = w[7] = 11 * npar + 1                     # p1 == p2
    slot = rng.permutation(npar + no).astype(np.int32)
    assert not np.array_equal(slot, np.arange(npar + no))
    R0 = np.full((npar + no, ld), SENT)
    R0[:, :n] = rng.uniform(-5, 5, size=(npar + no, n))
    want = R0.copy()
    crosses, same = set(), False
    for i in range(no):
        p1, p2, cross = int(w[3 * i]) % npar, int(w[3 * i + 1]) % npar, int(w[3 * i + 2]) % n
        crosses.add(cross)
        same |= p1 == p2
        want[slot[npar + i], :cross] = R0[slot[p1], :cross]
        want[slot[npar + i], cross:n] = R0[slot[p2], cross:n]
    assert 0 in crosses and n - 1 in crosses and same
    dw, ds, dR = DevBuf.from_array(w), DevBuf.from_array(slot), DevBuf.from_array(R0)
    assert L.nla_k_esch_crossover(n, ld, npar, no, dw.ptr, ds.ptr, dR.ptr, None) == 0
    assert L.nla_stream_sync(None) == 0
    got = dR.to_array(np.float64, (npar + no) * ld).reshape(npar + no, ld)
    assert np.array_equal(bits(got[slot[:npar]]), bits(R0[slot[:npar]]))          # parents
    assert np.array_equal(bits(got), bits(want))                                  # offspring exact, padding untouched


@pytest.mark.parametrize("n", [1, 256, 257, 513])
def test_gather_rows(L, n):
    rng = np.random.default_rng(200 + n)
    ld, rows, i0 = n + 3, 23, 7
    slot = rng.permutation(rows).astype(np.int32)
    R = rng.uniform(-5, 5, size=(rows, ld))
    R[3, 0] = -0.0
    dR, ds = DevBuf.from_array(R), DevBuf.from_array(slot)
    for count in (1, 5):
        G0 = np.full((count + 1, ld), SENT)
        want = G0.copy()
        want[:count, :n] = R[slot[i0:i0 + count], :n]
        dG = DevBuf.from_array(G0)
        assert L.nla_k_esch_gather_rows(n, ld, ds.ptr, i0, count, dR.ptr, dG.ptr, None) == 0
        assert L.nla_stream_sync(None) == 0
        assert np.array_equal(bits(dG.to_array(np.float64, (count + 1) * ld)), bits(want).ravel())
        dG.free()


@pytest.mark.parametrize("count", [1, 2, 255, 257, 5000, 70000])
def test_select_is_a_stable_sort(L, count):
    """(slot, fit) reordered by fitness as np.argsort(kind="stable") orders it: ties everywhere (16 levels), -0.0 and +0.0
    (equal: the index decides, and each keeps its sign bit), +-inf, denormals, negative values.  NaN is not part of this
    launcher's contract — the driver sorts on the host when a fitness is NaN — so none is passed."""
    rng = np.random.default_rng(300 + count)
    fit = (rng.integers(-8, 8, size=count) / 4.0).astype(np.float64)
    special = np.array([-0.0, 0.0, np.inf, -np.inf, 5e-324, -5e-324, 2.2e-308, -1e-310, 0.0, -0.0])
    where = rng.random(count) < 0.3
    fit[where] = special[rng.integers(0, len(special), size=int(where.sum()))]
    if count >= 2:
        fit[0], fit[count - 1] = 0.0, -0.0
    slot = rng.permutation(count).astype(np.int32) + 3
    order = np.argsort(fit, kind="stable")
    nb = L.nla_esch_sort_scratch_bytes(count)
    dscr, dsi, dfi = DevBuf(nb), DevBuf.from_array(slot), DevBuf.from_array(fit)
    dso, dfo = DevBuf.from_array(np.full(count + 1, -1, np.int32)), DevBuf.from_array(np.full(count + 1, SENT))
    assert L.nla_k_esch_select(count, dsi.ptr, dfi.ptr, dso.ptr, dfo.ptr, dscr.ptr, nb, None) == 0
    assert L.nla_stream_sync(None) == 0
    so, fo = dso.to_array(np.int32, count + 1), dfo.to_array(np.float64, count + 1)
    assert np.array_equal(so[:count], slot[order]) and so[count] == -1
    assert np.array_equal(bits(fo[:count]), bits(fit[order])) and fo[count] == SENT


# ---- the point-mutation chain (esch.c:207-218) ---------------------------------------------------------------------------
def chain_reference(W, M, total, n, npar, no, lb, ub, slot, R, random_words=True):
    """`total` steps from the first M words of W applied to R in place, one after the other: [iurand(no)] [iurand(n)] then
    2-word attempts until one is accepted.  Returns (complete steps the segment holds, capped at total; word position behind the
    last of them; mask of the elements written)."""
    npairs = M // 2
    ok, val = cauchy_attempts(W[:2 * npairs], random_words)
    acc = np.flatnonzero(ok)
    k = np.searchsorted(acc, np.arange(npairs + 2))              # next accepted attempt at or after pair h: acc[k[h]], -1: none
    nxt = np.append(acc, -1)[k].tolist()
    Wl, vl = W.tolist(), val.tolist()
    touched = np.zeros(R.shape, bool)
    p = steps = 0
    while steps < total:
        h = nxt[p // 2 + 1]                                      # attempts of the step that starts at word p begin at p + 2
        if h < 0:
            break
        io, ip = Wl[p] % no, Wl[p + 1] % n
        R[slot[npar + io], ip] = lb[ip] + (ub[ip] - lb[ip]) * vl[h]
        touched[slot[npar + io], ip] = True
        p = 2 * h + 2
        steps += 1
    return steps, p, touched


class Mutation:
    def __init__(self, n, npar, no, seed):
        rng = np.random.default_rng(seed)
        self.n, self.npar, self.no, self.ld = n, npar, no, n + 3
        self.lb, self.ub = np.linspace(-4.0, -1.0, n), np.linspace(2.0, 9.0, n)
        self.slot = rng.permutation(npar + no).astype(np.int32)
        self.R0 = np.full((npar + no, self.ld), SENT)
        self.R0[:, :n] = rng.uniform(-1, 2, size=(npar + no, n))
        self.dlb, self.dub, self.dslot = DevBuf.from_array(self.lb), DevBuf.from_array(self.ub), DevBuf.from_array(self.slot)
        self.dR = DevBuf.from_array(self.R0)
        self.dlast = DevBuf.from_array(np.full(no * n, 77, np.int32))          # scratch the launcher clears itself

    def launch(self, L, W, M, total):
        """on the rows as they stand on the device; returns (R, out)"""
        dW = DevBuf.from_array(W[:M])
        dscr = DevBuf(L.nla_esch_mut_scratch_bytes(M))
        dout = DevBuf.from_array(np.array([-5, -5], np.int64))
        assert L.nla_k_esch_mutate(dW.ptr, M, total, self.n, self.ld, self.npar, self.no, self.dlb.ptr, self.dub.ptr, self.dslot.ptr,
                                   self.dR.ptr, self.dlast.ptr, dscr.ptr, dout.ptr, None) == 0
        assert L.nla_stream_sync(None) == 0
        out = dout.to_array(np.int64, 2)
        R = self.dR.to_array(np.float64, self.R0.size).reshape(self.R0.shape)
        dW.free()
        dscr.free()
        return R, out

    def reference(self, W, M, total, random_words=True):
        R = self.R0.copy()
        steps, p, touched = chain_reference(W, M, total, self.n, self.npar, self.no, self.lb, self.ub, self.slot, R, random_words)
        return R, steps, p, touched

    def check_rows(self, R, Rref, touched):
        """the whole of R: elements no step wrote (parents, padding, the rest) bit for bit; written ones within 1e-10 — the value is
        lb + (ub - lb) v with v in [0, 1] from tan(): libm's deviation in v reaches the element multiplied by the side of the box"""
        assert not touched[self.slot[:self.npar]].any() and not touched[:, self.n:].any()
        assert np.array_equal(bits(R)[~touched], bits(self.R0)[~touched])
        scale = np.broadcast_to(np.concatenate([self.ub - self.lb, np.ones(self.ld - self.n)]), R.shape)
        d = np.abs(R - Rref)[touched]
        s = np.maximum(np.abs(Rref), scale)[touched]
        if len(d):
            MAXDEV["v"] = max(MAXDEV["v"], float((d / s).max()))
            print("largest relative deviation of v so far: %.3g" % MAXDEV["v"])
        assert np.all(d <= RTOL * s)

    def check(self, L, W, M, total, random_words=True):
        Rref, steps, p, touched = self.reference(W, M, total, random_words)
        assert steps == total, "the case's segment is meant to hold the whole chain"
        R, out = self.launch(L, W, M, total)
        self.check_rows(R, Rref, touched)
        assert min(int(out[0]), total) == total
        assert int(out[1]) == p
        return p


def driver_M(total):
    return int(total * 4.6) + 8192                               # esch_driver.c: 4.29 words expected per step


@pytest.mark.parametrize("n,npar,no,total", [(1, 2, 3, 1), (3, 4, 7, 2), (64, 2000, 3000, 19200), (512, 100, 200, 10240)])
def test_mutate_random_words_driver_sized_segment(L, n, npar, no, total):
    M = driver_M(total)
    assert driver_M(2) % 2 == 1                                  # (3, 4, 7, 2): an odd segment length
    Mutation(n, npar, no, 400 + n).check(L, stream(M), M, total)


def test_mutate_contention_every_block_writes_every_element(L):
    """six elements, 4000 steps over five blocks: "last step wins" is decided between blocks for every element"""
    total = 4000
    M = driver_M(total)
    m = Mutation(2, 3, 3, 500)
    p = m.check(L, stream(M), M, total)
    assert p > 4 * BLOCK


@pytest.mark.parametrize("n,no", [(29, 37), (64, 3000)])
def test_mutate_more_than_128_blocks(L, n, no):
    """132 blocks: esch_mut_chain_kernel's loop runs a second tile (with random words the 120 000 steps end in block 125 or so —
    the live chain across the tile edge is test_mutate_crafted_straddles_in_132_blocks)"""
    total, M = 120000, 540000
    p = Mutation(n, 5, no, 600 + n).check(L, stream(M), M, total)
    assert p > 100 * BLOCK


def test_mutate_exact_fit_too_short_and_retried(L):
    """M = where the serial chain stands after `total` steps: the chain fits to the last word.  Two words less: the launcher
    reports the complete steps the segment holds (< total; out[1] is then undefined and not looked at) and HAS applied them;
    the retry on the same rows with a longer segment leaves exactly what one correct pass over the original rows leaves — the
    contract esch_driver.c's `M *= 2` loop relies on."""
    n, npar, no, total = 5, 3, 11, 3000
    W = stream(40000)
    m = Mutation(n, npar, no, 700)
    Rref, steps, Mfit, touched = m.reference(W, 40000, total)
    assert steps == total and 3 * BLOCK < Mfit < 20000
    # exact fit (on fresh rows)
    e = Mutation(n, npar, no, 700)
    R, out = e.launch(L, W, Mfit, total)
    e.check_rows(R, Rref, touched)
    assert int(out[0]) >= total and int(out[1]) == Mfit
    # too short
    Rs_ref, short_steps, _, short_touched = m.reference(W, Mfit - 2, total)
    assert short_steps == total - 1
    R, out = m.launch(L, W, Mfit - 2, total)
    assert int(out[0]) == short_steps < total
    m.check_rows(R, Rs_ref, short_touched)                       # the complete steps were applied, with "last step wins" among them
    # ... then retried on the same rows
    R, out = m.launch(L, W, 2 * Mfit, total)
    m.check_rows(R, Rref, touched)
    assert min(int(out[0]), total) == total and int(out[1]) == Mfit


# crafted streams: acceptance independent of any libm — a rejected attempt has u in [0, 0.01] (|c| > 31), an accepted one u in
# [0.2, 0.8] (|c| < 1.4)
def pair_from_u(u):
    k = int(np.floor(u * 9007199254740992.0))
    return (k >> 26) << 5, (k & ((1 << 26) - 1)) << 6


def crafted_stream(M, straddles, seed, p_reject=0.18):
    """M words of whole steps; for every (boundary word B, exit offset off) in `straddles` one step starts at B - 6 and its
    rejected attempts carry it to B + off.  Returns the words and the number of steps in them."""
    rng = np.random.default_rng(seed)
    out = []

    def step(r):
        out.extend(int(x) for x in rng.integers(0, 1 << 32, size=2))
        for _ in range(r):
            out.extend(pair_from_u(rng.uniform(0.0, 0.01)))
        out.extend(pair_from_u(rng.uniform(0.2, 0.8)))

    steps = 0
    todo = sorted(straddles)
    while len(out) < M:
        if todo and len(out) >= todo[0][0] - 6 - 64:
            B, off = todo.pop(0)
            gap = B - 6 - len(out)
            assert gap >= 0 and gap % 2 == 0
            if gap % 4:
                step(1)
                steps += 1
                gap -= 6
            for _ in range(gap // 4):
                step(0)
                steps += 1
            assert len(out) == B - 6
            step((6 + off - 4) // 2)                             # 2 + 2 r + 2 words = 6 + off
            steps += 1
            assert len(out) == B + off
            continue
        r = 0
        while rng.random() < p_reject and r < 6:
            r += 1
        step(r)
        steps += 1
    return np.array(out, dtype=np.uint64).astype(np.uint32), steps


@pytest.mark.parametrize("off", [0, 2, 30, 62])
def test_mutate_crafted_straddle_of_the_first_block_boundary(L, off):
    """a step that starts 6 words before word 4096 and ends `off` words into block 1 (off = 62: 32 rejected attempts in a row,
    the largest exit offset the chain follows; 64 and beyond is outside the launcher's contract and is not run)"""
    W, nsteps = crafted_stream(3 * BLOCK, [(BLOCK, off)], 800 + off)
    total = nsteps - 3
    m = Mutation(7, 2, 9, 810 + off)
    p = m.check(L, W, len(W), total, random_words=False)
    assert p > 2 * BLOCK


def test_mutate_crafted_straddles_in_132_blocks(L):
    """540 000 crafted words whose 120 000 steps reach into block 128 and beyond: straddles at blocks 1 -> 2 and 127 -> 128 — the
    second crosses the tile edge of esch_mut_chain_kernel, whose second tile takes steps / entry offset over through LDS"""
    total, M = 120000, 540000
    W, nsteps = crafted_stream(M, [(2 * BLOCK, 30), (128 * BLOCK, 62), (129 * BLOCK, 2)], 900)
    assert nsteps >= total
    W = W[:M]
    m = Mutation(29, 5, 37, 910)
    p = m.check(L, W, M, total, random_words=False)
    assert p > 129 * BLOCK + 2
