"""-m gpu: the three device implementations of the ISRES evolve phase (mutation isres.c:234-252, differential variation :253-280) at
kernel level, behind the one contract of include/nlopt_amd.h (state[0] next individual, state[1] next deviate, state[2] ran out):

  isres_evolve_kernel      (hip/isres_kernels.hip, one wavefront; the launcher takes it for n > 1150)
  isres_evolve_lds_kernel  (same file, n <= 1150: a one-pass shift-map path for mutation individuals with n <= 256, a fix-point path)
  the multi-start rounds   (hip/isres_evolve2.hip: stage / scan with segment tail / chain / write, hand-over to the serial kernel)

against reference() below — the two loops written out in numpy.longdouble, one coordinate after the other, not the product's C code
and not oracle/emu_device.c (a second, independent statement: tests/test_isres_evolve_emulated.py passes this module over the emulated
device, and that agreement checks the reference and the harness).

What is exact and what is not.  Which deviate a coordinate uses, how often it is redrawn, where an individual starts and where the phase
ends are integers: compared exactly.  X and S pass through the device's exp and possibly a contracted multiply-add in its argument: about
3e-15 relative on sigma', times |z| <= 6 and, in the variation phase, a chain of at most a few dozen survivors — X within
1e-12 (ub_j - lb_j), S within 1e-12 max(|S_ref|, |S_parent|).  A draw within rounding of a bound could be accepted by one side and
redrawn by the other, so every case asserts FIRST that the reference never tested a value closer than MARGIN = 1e-9 (relative to the
box) to a bound; no case is left out for it (the seeds below satisfy it).  The implementations must agree with each other bit for bit.

Untouched memory: the padding columns (ld = (n + 1) & ~1), every row the phase does not write — the survivors' rows in the mutation
phase, the other rows in the variation phase — and, after a run-out, every row of an individual not yet finished must come back
bit-identical.  Rows that the phase never reads (the children's before the mutation, rows at and beyond `survivors` that no survivor
owns in the variation phase) are uploaded as sentinels.

Device-only checks, skipped over the emulated device (which defines them away): that a hand-over happened, the count of rounds
(state[11]), nla_k_isres_evolve_parent_mu, nla_isres_evolve2_supported."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import nlopt_amd
from nlopt_amd import DevBuf

pytestmark = pytest.mark.gpu
EMU = bool(os.environ.get("NLA_TEST_EMU_DEVICE"))
LD = np.longdouble
MARGIN = 1e-9
XTOL = 1e-12
STOL = 1e-12
SENT = -7.25
MAXN = 1150
vp, i32, i64, f64 = C.c_void_p, C.c_int, C.c_int64, C.c_double


@pytest.fixture(scope="module")
def L():
    L = nlopt_amd.lib()
    assert nlopt_amd.device_count() > 0, "no HIP device: the product has no CPU fallback"
    return L


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def reference(n, phase, pop, survivors, z, zcount, irank, X, S, lb, ub, taup, tau, x0c, k, pos, kend=None):
    """isres.c:234-280 from individual k, deviate pos, with the deviates z[0 .. zcount).  X, S: pop x n.  An individual is written only
    if every deviate it reads has an index < zcount (before each mutated coordinate: cur + 1 >= zcount means ran out).
    Returns a dict: X, S (longdouble), start[k] / used[k] / redraws[k] per finished individual, draws[k] = [(j, index of the coordinate's
    sigma deviate)], redrawn = indices of the deviates read as redraws, k, pos, ranout, margin."""
    X = np.array(X, dtype=LD)
    S = np.array(S, dtype=LD)
    lb, ub, zl, x0c = np.array(lb, dtype=LD), np.array(ub, dtype=LD), np.array(z, dtype=LD), np.array(x0c, dtype=LD)
    w = ub - lb
    smax = w / np.sqrt(LD(n))
    taup, tau, ALPHA, GAMMA = LD(taup), LD(tau), LD(0.2), LD(0.85)
    if kend is None:
        kend = pop if phase == 0 else survivors
    out = dict(start={}, used={}, redraws={}, draws={}, redrawn=[], margin=np.inf, ranout=0)

    def inside(x, j, count):
        if count and w[j] > 0:
            out["margin"] = min(out["margin"], float(min(abs(x - lb[j]), abs(x - ub[j])) / w[j]))
        return not (x < lb[j] or x > ub[j])

    with np.errstate(over="ignore"):
        while k < kend:
            rk = int(irank[k])
            ri = int(irank[k % survivors]) if phase == 0 else rk
            last = k + 1 == survivors
            if pos >= zcount:
                out["ranout"] = 1
                break
            taup_rand = taup * zl[pos]
            cur = pos + 1
            xo, so, draws, nred = X[ri].copy(), S[ri].copy(), [], 0
            for j in range(n):
                xi, si = X[ri, j], S[ri, j]
                mutate = True
                if phase == 1:
                    if not last:
                        xo[j] = xi + GAMMA * (x0c[j] - X[k + 1, j])          # the CURRENT physical row k + 1 (isres.c:260)
                        mutate = not inside(xo[j], j, True)
                if mutate:
                    if cur + 1 >= zcount:
                        out["ranout"] = 1
                        break
                    sg = si * np.exp(taup_rand + tau * zl[cur])
                    if sg > smax[j]:
                        sg = smax[j]
                    t = 1
                    while True:
                        if cur + t >= zcount:
                            out["ranout"] = 1
                            break
                        if t > 1:
                            out["redrawn"].append(cur + t)
                        xn = xi + sg * zl[cur + t]
                        if inside(xn, j, sg != 0):
                            break
                        t += 1
                    if out["ranout"]:
                        break
                    xo[j], so[j] = xn, si + ALPHA * (sg - si)
                    draws.append((j, cur))
                    nred += t - 1
                    cur += 1 + t
            if out["ranout"]:
                break
            X[rk], S[rk] = xo, so
            out["start"][k], out["used"][k], out["redraws"][k], out["draws"][k] = pos, cur - pos, nred, draws
            pos = cur
            k += 1
    out.update(X=X, S=S, k=k, pos=pos)
    return out


# ---- populations -----------------------------------------------------------------------------------------------------------------
class Case:
    """one population: bounds that differ per coordinate, a random ranking, deviates; kind "wide": x uniform in the box, sigma 5 % of
    the cap (ub - lb) / sqrt(n) — few redraws; "bound": every coordinate within 1e-3 of a bound, sigma at the cap — about one redraw
    per coordinate"""

    def __init__(self, n, pop, survivors, kind, seed=0, fixed=None, irank=None, pos0=None, zextra=0, zseed=None):
        rng = np.random.default_rng([n, pop, survivors, kind == "bound", seed])
        self.n, self.pop, self.survivors, self.kind, self.ld = n, pop, survivors, kind, (n + 1) & ~1
        self.lb = -1.0 - 3.0 * rng.random(n)
        self.ub = 0.5 + 2.0 * rng.random(n)
        w = self.ub - self.lb
        cap = w / math.sqrt(n)
        if kind == "wide":
            self.X = self.lb + w * rng.random((pop, n))
            self.S = np.tile(0.05 * cap, (pop, 1))
        else:
            u, low = 1e-3 * rng.random((pop, n)), rng.random((pop, n)) < 0.5
            self.X = np.where(low, self.lb + u * w, self.ub - u * w)
            self.S = np.tile(cap, (pop, 1))
        if fixed is not None:                                        # lb == ub, x on it, sigma 0 (what nla_k_isres_init gives it)
            self.ub[fixed] = self.lb[fixed]
            self.X[:, fixed] = self.lb[fixed]
            self.S[:, fixed] = 0.0
        self.irank = rng.permutation(pop).astype(np.int32) if irank is None else np.asarray(irank, dtype=np.int32)
        assert sorted(self.irank.tolist()) == list(range(pop))
        self.taup, self.tau = 1.0 / math.sqrt(2.0 * n), 1.0 / math.sqrt(2.0 * math.sqrt(n))
        self.pos0 = (3 if n % 2 else 1000) if pos0 is None else pos0
        self.z = rng.standard_normal(self.pos0 + pop * (1 + 5 * n) + 4096 + zextra)
        if zseed is not None:                                        # the same population with other deviates
            self.z = np.random.default_rng([n, zseed]).standard_normal(len(self.z))
        self._ref = {}

    def span(self, phase):
        return (self.survivors, self.pop) if phase == 0 else (0, self.survivors)

    def inputs(self, phase):
        """X, S (pop x n) as uploaded for this phase: rows the phase never reads hold sentinels"""
        X, S = self.X.copy(), self.S.copy()
        if phase == 0:
            rows = self.irank[self.survivors:]
        else:
            rows = np.array([r for r in self.irank[self.survivors:] if r >= self.survivors and r != 0], dtype=np.int64)
        X[rows] = SENT
        S[rows] = SENT
        return X, S

    def ref(self, phase, z=None, zcount=None):
        key = (phase, zcount) if z is None else None
        if key is not None and key in self._ref:
            return self._ref[key]
        zz = self.z if z is None else z
        X, S = self.inputs(phase)
        r = reference(self.n, phase, self.pop, self.survivors, zz, len(zz) if zcount is None else zcount, self.irank, X, S, self.lb, self.ub,
                      self.taup, self.tau, X[0], self.span(phase)[0], self.pos0)
        if key is not None:
            self._ref[key] = r
        return r


_cases = {}


def case(n, pop, survivors, kind, **kw):
    key = (n, pop, survivors, kind, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _cases:
        _cases[key] = Case(n, pop, survivors, kind, **kw)
    return _cases[key]


# ---- the harness: the driver's protocol (isres_driver.c:420-473) for one phase -----------------------------------------------------
_ws = {}


def workspace(L, n):
    need = int(L.nla_isres_evolve2_ws_bytes(n))
    if "b" not in _ws or _ws["b"].nbytes < need:
        if "b" in _ws:
            _ws["b"].free()
        _ws["b"] = DevBuf(need)
    return _ws["b"]


class Phase:
    """uploads a case's inputs for one phase and plays the rounds / refill / hand-over protocol with the "serial" kernel
    (nla_k_isres_evolve) or the "rounds" (nla_k_isres_evolve_rounds, handing single individuals to the serial kernel)"""

    def __init__(self, L, c, impl, phase, z=None, rho=(0, 0, 0, 0), mu="computed"):
        self.L, self.c, self.impl, self.phase = L, c, impl, phase
        n, ld, pop = c.n, c.ld, c.pop
        X, S = c.inputs(phase)
        self.X0 = np.full((pop, ld), SENT)
        self.S0 = np.full((pop, ld), SENT)
        self.X0[:, :n], self.S0[:, :n] = X, S
        z = c.z if z is None else z
        self.zlen = len(z)
        self.kend = c.span(phase)[1]
        self.state = np.zeros(16, dtype=np.int64)
        self.state[0], self.state[1] = c.span(phase)[0], c.pos0
        # 1. the inputs
        self.dX, self.dS, self.dz = DevBuf.from_array(self.X0), DevBuf.from_array(self.S0), DevBuf.from_array(z)
        self.dlb, self.dub, self.dirank = DevBuf.from_array(c.lb), DevBuf.from_array(c.ub), DevBuf.from_array(c.irank)
        self.dscratch = DevBuf.from_array(np.full(3 * ld, SENT))
        self.dstate = DevBuf.from_array(self.state)
        self.handed, self.calls = [], 0
        if impl == "rounds":
            self.dinv = DevBuf.from_array(np.full(pop, -1, dtype=np.int32))
            self.drho = DevBuf.from_array(np.asarray(rho, dtype=np.float64))
            self.dmu = DevBuf.from_array(np.zeros(max(c.survivors, 1)) if mu in ("computed", "zero") else np.full(max(c.survivors, 1), float(mu)))
            self.ws = workspace(L, n)
            assert L.nla_k_isres_inverse(pop, self.dirank.ptr, self.dinv.ptr, None) == 0                      # 2.
            if phase == 0 and mu == "computed":                                                              # 3.
                assert L.nla_k_isres_evolve_parent_mu(n, ld, c.survivors, self.dlb.ptr, self.dub.ptr, self.dirank.ptr, self.dX.ptr, self.dS.ptr,
                                                      self.dmu.ptr, None) == 0
            if phase == 1:                                                                                   # 4. memcpy(x0, xs, n), isres.c:253
                assert L.nla_memcpy_d2d(self.dscratch.ptr, self.dX.ptr, 8 * n, None) == 0
            assert L.nla_stream_sync(None) == 0

    def _up(self):
        assert self.L.nla_memcpy_h2d(self.dstate.ptr, self.state.ctypes.data, self.state.nbytes, None) == 0 and self.L.nla_stream_sync(None) == 0

    def _down(self):
        self.state = self.dstate.to_array(np.int64, 16)

    def _serial(self, zcount):
        c = self.c
        assert self.L.nla_k_isres_evolve(c.n, c.ld, self.phase, c.pop, c.survivors, zcount, c.taup, c.tau, self.dlb.ptr, self.dub.ptr, self.dz.ptr,
                                         self.dirank.ptr, self.dX.ptr, self.dS.ptr, self.dscratch.ptr, self.dstate.ptr, None) == 0

    def play(self, zcount=None, rounds=3, refill=None):
        """5. the loop; when the deviates run out: stop (refill None) or go on with `refill` deviates.  Called again after a stop it resumes
        (the driver's refill: clear state[2], more deviates)."""
        c, st = self.c, self.state
        zcount = self.zlen if zcount is None else zcount
        if st[2]:
            st[2] = 0
            self._up()
        for _ in range(20000):
            if self.impl == "rounds":
                assert self.L.nla_k_isres_evolve_rounds(c.n, c.ld, self.phase, c.pop, c.survivors, zcount, c.taup, c.tau, self.dlb.ptr, self.dub.ptr,
                                                        self.dz.ptr, self.dirank.ptr, self.dinv.ptr, self.dX.ptr, self.dS.ptr, self.dscratch.ptr,
                                                        self.dstate.ptr, self.drho.ptr, self.ws.ptr, self.dmu.ptr, rounds, None) == 0
            else:
                self._serial(zcount)
            self.calls += 1
            self._down()
            st = self.state
            if not st[2] and self.impl == "rounds" and st[10]:           # one individual the look-up could not resolve
                self.handed.append(int(st[0]))
                st[10], st[14] = 0, st[0] + 1
                self._up()
                self._serial(zcount)
                self._down()
                st = self.state
                st[14] = 0
                if st[2]:
                    st[10] = 1                                           # ran out inside the serial step: it is taken again after the refill
                self._up()
            if st[2]:
                if refill is None:
                    return self
                zcount, refill = refill, None
                st[2] = 0
                self._up()
                continue
            if self.impl == "serial" or st[0] >= self.kend:
                return self
        raise AssertionError("the phase does not end: state %s" % st)

    def result(self):
        c = self.c
        X = self.dX.to_array(np.float64, c.pop * c.ld).reshape(c.pop, c.ld)
        S = self.dS.to_array(np.float64, c.pop * c.ld).reshape(c.pop, c.ld)
        return X, S, self.state.copy(), int(self.state[11]), len(self.handed)


def run(L, c, impl, phase, **kw):
    play = {k: kw.pop(k) for k in ("zcount", "rounds", "refill") if k in kw}
    p = Phase(L, c, impl, phase, **kw).play(**play)
    return p.result() + (p,)


def check(c, phase, ref, X, S, state, label, upto=None):
    """X, S (pop x ld, from the device) against the reference for the individuals before `upto` (default: the whole phase); everything
    else bit-identical to what was uploaded"""
    n = c.n
    k0, kend = c.span(phase)
    upto = kend if upto is None else upto
    Xin, Sin = c.inputs(phase)
    X0, S0 = np.full((c.pop, c.ld), SENT), np.full((c.pop, c.ld), SENT)
    X0[:, :n], S0[:, :n] = Xin, Sin
    written = np.zeros((c.pop, c.ld), dtype=bool)
    w = c.ub - c.lb
    dx = ds = 0.0
    for k in range(k0, upto):
        rk = int(c.irank[k])
        ri = int(c.irank[k % c.survivors]) if phase == 0 else rk
        written[rk, :n] = True
        ex = np.abs(X[rk, :n].astype(LD) - ref["X"][rk]).astype(np.float64)
        es = np.abs(S[rk, :n].astype(LD) - ref["S"][rk]).astype(np.float64)
        sscale = np.maximum(np.abs(ref["S"][rk].astype(np.float64)), np.abs(Sin[ri]))
        assert np.all(ex <= XTOL * w), (label, "X of individual", k, "coordinate", int(np.argmax(ex - XTOL * w)), float(ex.max()))
        assert np.all(es <= STOL * sscale), (label, "S of individual", k, "coordinate", int(np.argmax(es - STOL * sscale)), float(es.max()))
        dx = max(dx, float(np.max(ex[w > 0] / w[w > 0])) if np.any(w > 0) else 0.0)
        ds = max(ds, float(np.max(es[sscale > 0] / sscale[sscale > 0])) if np.any(sscale > 0) else 0.0)
    for name, got, want in (("X", X, X0), ("S", S, S0)):
        bad = (bits(got) != bits(want)) & ~written
        assert not bad.any(), (label, name, "changed outside the rows of the finished individuals: (row, column)", np.argwhere(bad)[:4].tolist())
    return dx, ds


def against_reference(L, c, phase, label, impls=("serial", "rounds"), **kw):
    """items 1 and 2: every implementation against the reference, and the implementations against each other bit for bit"""
    ref = c.ref(phase) if "z" not in kw else c.ref(phase, z=kw["z"])
    assert not ref["ranout"] and ref["k"] == c.span(phase)[1], "the test's own deviates do not suffice"
    assert ref["margin"] >= MARGIN, (label, "reference margin", ref["margin"])
    res = {}
    for impl in impls:
        X, S, st, nrounds, nhand, p = run(L, c, impl, phase, **kw)
        assert st[0] == c.span(phase)[1] and st[2] == 0, (label, impl, st)
        assert st[1] == ref["pos"], (label, impl, "deviates consumed", int(st[1]), "reference", ref["pos"])
        dx, ds = check(c, phase, ref, X, S, st, "%s %s" % (label, impl))
        print("DEV %-46s %-6s phase %d: max |dX|/(ub-lb) %.3g  max |dS|/scale %.3g  margin %.3g  rounds %d hand-overs %d"
              % (label, impl, phase, dx, ds, ref["margin"], nrounds, nhand))
        res[impl] = (X, S, st, nrounds, p)
    if len(res) == 2:
        a, b = res["serial"], res["rounds"]
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1])) and a[2][1] == b[2][1], (label, "rounds != serial")
    return ref, res


# ---- 1, 2: against the reference; rounds == serial bit for bit ---------------------------------------------------------------------
SHAPES = [(1, 1300, 200), (3, 1400, 300), (2, 40, 39), (63, 120, 20), (64, 120, 20), (65, 120, 20), (255, 60, 9), (256, 60, 9), (257, 60, 9),
          (1150, 24, 4), (1151, 12, 2),
          (7, 30, 1),                                        # survivors == 1
          (6, 40, 25), (6, 40, 24), (6, 40, 23)]             # pop - survivors = 15, 16, 17: a segment of children, one less, one more


@pytest.mark.parametrize("phase", [0, 1])
@pytest.mark.parametrize("kind", ["wide", "bound"])
@pytest.mark.parametrize("n,pop,survivors", SHAPES)
def test_against_reference(L, n, pop, survivors, kind, phase):
    c = case(n, pop, survivors, kind)
    against_reference(L, c, phase, "%s n=%d pop=%d surv=%d" % (kind, n, pop, survivors), impls=("serial", "rounds") if n <= MAXN else ("serial",))


@pytest.mark.parametrize("phase", [0, 1])
@pytest.mark.parametrize("kind", ["wide", "bound"])
def test_fixed_coordinate(L, kind, phase):
    """lb_j == ub_j, x on it, sigma 0: the coordinate stays exactly where it is and its draws are consumed like any other's"""
    c = case(9, 50, 8, kind, fixed=4)
    ref, res = against_reference(L, c, phase, "%s n=9 fixed coordinate 4" % kind)
    for impl, r in res.items():
        k0, kend = c.span(phase)
        assert np.all(r[0][c.irank[k0:kend], 4] == c.lb[4]), impl


# ---- 3: predictions never change results -------------------------------------------------------------------------------------------
PRED = [("bound", 65, 120, 20), ("bound", 1150, 24, 4), ("wide", 3, 1400, 300)]
# bound, n = 1150 makes 1117 +- 49 redraws per individual, and even from its exact start an individual has room for n + 192 in the scan's
# window: deviate seeds (per phase) on which one individual exceeds n + 200 — found by a search in float64, asserted through the reference
HEAVY_ZSEED = {0: 123715, 1: 216449}


@pytest.mark.parametrize("phase", [0, 1])
@pytest.mark.parametrize("kind,n,pop,survivors", PRED)
def test_predictions_never_change_results(L, kind, n, pop, survivors, phase):
    """the running redraw statistics rho, the per-parent expectation mu_rp and the number of rounds enqueued per call only say where the
    scan looks: a wrong one costs rounds, never a different result.  On bound n = 1150 an individual leaves the window whatever is
    predicted from its exact start: the rounds as the driver plays them hand it to the serial kernel."""
    c = case(n, pop, survivors, kind, zseed=HEAVY_ZSEED[phase]) if n == 1150 else case(n, pop, survivors, kind)
    label = "%s n=%d pop=%d predictions" % (kind, n, pop)
    ref, res = against_reference(L, c, phase, label, impls=("rounds",))
    heavy = [k for k, r in ref["redraws"].items() if r > n + 200]
    assert heavy or n != 1150, "the deviate seed gives no individual with more than n + 200 redraws"
    X0, S0, st0 = res["rounds"][:3]
    for kw in (dict(rho=(1e6, 1, 1e6, 1)), dict(rho=(0, 1e6, 0, 1e6)), dict(mu="zero"), dict(mu=1e4), dict(rounds=1), dict(rounds=72)):
        X, S, st, nrounds, nhand, _ = run(L, c, "rounds", phase, **kw)
        print("DEV %-46s phase %d %s: rounds %d hand-overs %d" % (label, phase, kw, nrounds, nhand))
        assert st[0] == st0[0] and st[1] == st0[1] and st[2] == 0, (kw, st)
        assert np.array_equal(bits(X), bits(X0)) and np.array_equal(bits(S), bits(S0)), kw
    if n == 1150 and not EMU:
        # (with rho zero, mu_rp as computed, 3 rounds a call; a prediction that puts the start early in its window leaves more room, so not
        # every variation must hand over)
        assert set(heavy) <= set(res["rounds"][4].handed), (heavy, res["rounds"][4].handed)


# ---- 4: the deviates run out and the phase resumes ---------------------------------------------------------------------------------
# (n = 1151: the one-wavefront kernel, which the rounds never call)
RUNOUT = [(n, pop, s, impl) for n, pop, s in ((5, 70, 10), (300, 20, 3)) for impl in ("serial", "rounds")] + [(1151, 12, 2, "serial")]


@pytest.mark.parametrize("phase", [0, 1])
@pytest.mark.parametrize("kind", ["wide", "bound"])
@pytest.mark.parametrize("n,pop,survivors,impl", RUNOUT)
def test_deviates_run_out_and_the_phase_resumes(L, n, pop, survivors, impl, kind, phase):
    c = case(n, pop, survivors, kind, pos0=0)
    k0, kend = c.span(phase)
    base = c.ref(phase)
    mid = k0 + (kend - k0) // 2
    # a redraw run of three in the middle of the phase: where some individual from `mid` on draws its first mutated coordinate
    kb = next(k for k in range(mid, kend) if base["draws"][k])
    at = base["draws"][kb][0][1] + 1
    z = c.z.copy()
    z[at:at + 3] = 1e6
    full = c.ref(phase, z=z)
    label = "%s n=%d run-out" % (kind, n)
    assert full["margin"] >= MARGIN and not full["ranout"] and set(range(at + 1, at + 4)) <= set(full["redrawn"]), label
    p_end, pk = full["pos"], full["start"][mid]
    whole = Phase(L, c, impl, phase, z=z).play()
    Xw, Sw, stw = whole.result()[:3]
    assert stw[0] == kend and stw[1] == p_end and stw[2] == 0
    check(c, phase, full, Xw, Sw, stw, label + " " + impl)
    Xin = whole.X0
    for zc in (0, 1, pk + 1, pk + 2, at + 2, p_end - 1, p_end):
        r = c.ref(phase, z=z, zcount=zc)
        assert r["margin"] >= MARGIN
        p = Phase(L, c, impl, phase, z=z).play(zcount=zc)
        X, S, st = p.result()[:3]
        if zc == p_end:
            assert st[0] == kend and st[2] == 0 and st[1] == p_end, (zc, st)
        else:
            assert r["ranout"] == 1 and st[2] == 1, (zc, st)
            assert st[0] == r["k"] if impl == "serial" else k0 <= st[0] <= r["k"], (zc, st, r["k"])
            assert st[1] == (full["start"][int(st[0])]), (zc, st)
            check(c, phase, full, X, S, st, "%s %s zcount=%d" % (label, impl, zc), upto=int(st[0]))   # unfinished rows: bit-identical to the input
            p.play()                                                                                    # the refill: all deviates
            X, S, st = p.result()[:3]
            assert st[0] == kend and st[2] == 0 and st[1] == p_end, (zc, st)
        assert np.array_equal(bits(X), bits(Xw)) and np.array_equal(bits(S), bits(Sw)), (label, impl, "resumed after zcount", zc)
        assert np.array_equal(bits(p.X0), bits(Xin))


# ---- 5: crafted redraw bursts ------------------------------------------------------------------------------------------------------
def burst_case(n, phase, slot, kind):
    """phase 0: 22 children, the first of the block (slot 0) and the one at slot 17.  phase 1: every coordinate of the chosen survivor must
    mutate — slot 17 is the last of 18 survivors (isres.c:262), slot 0 a first survivor whose differential step leaves the box everywhere"""
    if phase == 0 or slot == 17:
        return case(n, 40, 18, kind, zextra=4096)
    key = ("burst0", n, kind)
    if key not in _cases:
        c = Case(n, 40, 18, kind, seed=1, zextra=4096)
        if c.irank[0] in (0, 1):
            q = int(np.argmax(c.irank > 1))
            c.irank[[0, q]] = c.irank[[q, 0]]
        w = c.ub - c.lb
        c.X[0], c.X[1], c.X[c.irank[0]] = c.lb + 0.9 * w, c.lb + 0.1 * w, c.lb + 0.5 * w      # 0.5 + 0.85 (0.9 - 0.1) = 1.18: outside
        _cases[key] = c
    return _cases[key]


BURSTS = [(n, B) for n in (1, 40, 300) for B in (n + 63, n + 66, n + 200)] + [(1, 400), (40, 400)]


@pytest.mark.parametrize("phase", [0, 1])
@pytest.mark.parametrize("kind", ["wide", "bound"])
@pytest.mark.parametrize("n,B", BURSTS)
def test_redraw_bursts(L, n, B, kind, phase):
    """B deviates of 1e6 where an individual draws a coordinate: B redraws there.  n + 63 still fits the serial LDS kernel's window of
    3n + 64 deviates, n + 66 does not (and leaves the one-pass band of a mutation individual with n <= 256); n + 200 and 400 do not fit
    the scan's window either, even from the exact start: the rounds hand the individual over.  On `bound` the natural redraws come on top."""
    for slot in (0, 17):
        c = burst_case(n, phase, slot, kind)
        k = c.span(phase)[0] + slot
        draws = c.ref(phase)["draws"][k]
        assert len(draws) == n, "the chosen individual mutates every coordinate"
        assert np.all(c.inputs(phase)[1][c.irank[: c.survivors]] >= 1e-3 * (c.ub - c.lb))
        for j in sorted({0, n // 2, n - 1}):
            at = draws[j][1] + 1
            z = c.z.copy()
            z[at:at + B] = 1e6
            label = "%s n=%d burst %d at individual %d coordinate %d" % (kind, n, B, k, j)
            ref, res = against_reference(L, c, phase, label, z=z)
            assert ref["redraws"][k] >= B
            if B >= n + 200 and not EMU:
                assert k in res["rounds"][4].handed, (label, res["rounds"][4].handed)


# ---- 6: variation dependencies -----------------------------------------------------------------------------------------------------
def dep_irank(which, pop, survivors, rng):
    ir = rng.permutation(pop)
    if which == "identity":
        ir = np.arange(pop)
    elif which == "own row is row k+1":
        ir = (np.arange(pop) + 1) % pop
    elif which == "waits for the one before":
        ir = (np.arange(pop) + 2) % pop
    elif which == "boundaries":
        for k in (1, 15, 16, 17, 31, 32, 255, 256):                # irank[k-1] = k+1 exactly there: individual k reads the row individual k-1 has just written
            q = int(np.where(ir == k + 1)[0][0])
            ir[[q, k - 1]] = ir[[k - 1, q]]
        at = (1, 15, 16, 17, 31, 32, 255, 256)
        for k in range(1, survivors):                              # ... and nowhere else: a chance one goes to the last non-survivor's place
            if ir[k - 1] == k + 1 and k not in at:
                ir[[k - 1, pop - 1]] = ir[[pop - 1, k - 1]]
        assert [k for k in range(1, survivors) if ir[k - 1] == k + 1] == list(at)
    elif which == "a survivor owns row 0":
        q = int(np.where(ir == 0)[0][0])
        ir[[q, 3]] = ir[[3, q]]
    elif which == "row `survivors` rewritten early":
        q = int(np.where(ir == survivors)[0][0])
        ir[[q, 2]] = ir[[2, q]]
    return ir.astype(np.int32)


DEPS = [("identity", 60, 20), ("own row is row k+1", 60, 20), ("waits for the one before", 60, 40), ("boundaries", 700, 300),
        ("a survivor owns row 0", 60, 20), ("row `survivors` rewritten early", 60, 20)]


@pytest.mark.parametrize("kind", ["wide", "bound"])
@pytest.mark.parametrize("n", [4, 70])
@pytest.mark.parametrize("which,pop,survivors", DEPS)
def test_variation_dependencies(L, which, pop, survivors, n, kind):
    """isres.c:260 reads the CURRENT physical row k + 1 — rewritten or not by an earlier survivor — and x0 is the snapshot of row 0 taken
    before the loop (:253)"""
    ir = dep_irank(which, pop, survivors, np.random.default_rng([n, pop, len(which)]))
    c = case(n, pop, survivors, kind, irank=ir, seed=len(which))
    ref, res = against_reference(L, c, 1, "%s n=%d %s" % (kind, n, which))
    if which == "waits for the one before" and not EMU:
        assert res["rounds"][3] >= 39, "a round resolved more than one survivor of a chain of dependencies"


# ---- 7: the helper kernels, the refusals -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pop", [1, 255, 256, 257])
def test_inverse(L, pop):
    ir = np.random.default_rng(pop).permutation(pop).astype(np.int32)
    dinv = DevBuf.from_array(np.full(pop + 2, -5, dtype=np.int32))
    dir_ = DevBuf.from_array(ir)
    assert L.nla_k_isres_inverse(pop, dir_.ptr, dinv.ptr, None) == 0 and L.nla_stream_sync(None) == 0
    inv = dinv.to_array(np.int32, pop + 2)
    assert np.array_equal(inv[ir], np.arange(pop)) and np.all(inv[pop:] == -5)


@pytest.mark.skipif(EMU, reason="device only: the emulated device needs no prediction")
@pytest.mark.parametrize("survivors", [1, 9])
@pytest.mark.parametrize("n", [1, 256, 257])
def test_parent_mu(L, n, survivors):
    """mu_rp[p] = sum_j q / (1 - q), q = (erfc((x - lb) / (sigma sqrt 2)) + erfc((ub - x) / (sigma sqrt 2))) / 2, capped at q = 0.999
    (999 per coordinate).  The cap bounds what an ulp of erfc is amplified by to 1e3: relative 1e-9."""
    for kind in ("wide", "bound"):
        c = Case(n, survivors + 5, survivors, kind, seed=3)
        c.S[c.irank[survivors - 1], ::3] = 1e7 * (c.ub - c.lb)[::3]              # draws that nearly always miss the box: q >= 0.999, the cap
        c.S[c.irank[0], n // 2::3] = 0.0                                          # sigmas of 0 (the last word where both meet)
        ld = c.ld
        X, S = np.full((c.pop, ld), SENT), np.full((c.pop, ld), SENT)
        X[:, :n], S[:, :n] = c.X, c.S
        dX, dS, dlb, dub, dir_ = (DevBuf.from_array(a) for a in (X, S, c.lb, c.ub, c.irank))
        dmu = DevBuf.from_array(np.full(survivors + 2, SENT))
        assert L.nla_k_isres_evolve_parent_mu(n, ld, survivors, dlb.ptr, dub.ptr, dir_.ptr, dX.ptr, dS.ptr, dmu.ptr, None) == 0
        assert L.nla_stream_sync(None) == 0
        mu = dmu.to_array(np.float64, survivors + 2)
        capped = False
        for p in range(survivors):
            r = int(c.irank[p])
            want = 0.0
            for j in range(n):
                inv = 0.7071067811865476 / max(c.S[r, j], 1e-300)
                q = 0.5 * (math.erfc((c.X[r, j] - c.lb[j]) * inv) + math.erfc((c.ub[j] - c.X[r, j]) * inv))
                capped |= q >= 0.999
                want += q / (1.0 - q) if q < 0.999 else 999.0
            assert abs(mu[p] - want) <= 1e-9 * want, (kind, p, mu[p], want)
        assert np.all(mu[survivors:] == SENT)
    assert capped or (n == 1 and survivors == 1)


@pytest.mark.skipif(EMU, reason="device only: the emulated device takes its answer from the environment")
def test_supported(L):
    assert [L.nla_isres_evolve2_supported(n) for n in (0, 1, 1150, 1151)] == [0, 1, 1, 0]


@pytest.mark.parametrize("n,phase,with_mu", [(1151, 0, True), (1151, 1, True), (8, 0, False)])
def test_refusals(L, n, phase, with_mu):
    """n beyond the rounds' staging limit, or a mutation phase without the parents' expectations: an error, and nothing is touched"""
    c = case(n, 12, 2, "wide")
    p = Phase(L, c, "serial", phase)                                              # (uploads only)
    st = np.arange(100, 116, dtype=np.int64)
    dst, dws, dinv, drho, dmu = DevBuf.from_array(st), DevBuf(1 << 16), DevBuf.from_array(np.zeros(c.pop, dtype=np.int32)), DevBuf.from_array(np.zeros(4)), DevBuf.from_array(np.zeros(2))
    rc = L.nla_k_isres_evolve_rounds(c.n, c.ld, phase, c.pop, c.survivors, p.zlen, c.taup, c.tau, p.dlb.ptr, p.dub.ptr, p.dz.ptr, p.dirank.ptr, dinv.ptr,
                                     p.dX.ptr, p.dS.ptr, p.dscratch.ptr, dst.ptr, drho.ptr, dws.ptr, dmu.ptr if with_mu else None, 3, None)
    assert L.nla_stream_sync(None) == 0
    assert rc != 0
    assert np.array_equal(dst.to_array(np.int64, 16), st)
    X, S = p.result()[:2]
    assert np.array_equal(bits(X), bits(p.X0)) and np.array_equal(bits(S), bits(p.S0))
