"""-m gpu: the CRS2_LM launchers crs_pass.c calls on its usual path, one by one, against the CPU oracle's statements of the same
contracts (oracle/port_kernels.c) through the kernel-level C-ABI — tests/test_gpu_kernels.py drives the pointer forms only.
  A  lists as kernel arguments: nla_k_crs_advance_args / _finish_args / _commit_args, and bit-identity with the pointer forms
  B  the fused commit with forwarding: nla_k_crs_advance_commit_args
  C  nla_k_crs_finish_args_bell; nla_k_crs_finish for obj = -1, obj = -2 and a negated objective
  D  the production form of the window launch: nla_k_crs_commit_zero + nla_k_crs_chain_lean (chain_kernel_case, lean mode)
  E  nla_k_crs_mutate
  F  the column-sharded pass on one device: nla_k_crs_sh_init_rows, _advance_cols, _sh_mutate_pack, _sh_eval, _commit_sh
The comparison rule is test_gpu_kernels.py's: whatever is copied, selected or formed by IEEE adds and multiplies is bit for bit the
sequential statement's; objective values are within RTOL = 1e-10 (device libm against glibc).  The column-slice expectations are
the WHOLE-ROW statements sliced in numpy, the fused commit's "commit applied to a host copy of X, then the whole-row statement":
the emulated device layer (tests/test_crs_launchers_emulated.py runs this module over it) is built from the column statements,
so those would prove nothing there.  Every refusal case returns from the launcher before anything is launched."""
import ctypes as C
import itertools

import numpy as np
import pytest

import _oracle as O
import nlopt_amd
from nlopt_amd import DevBuf
from test_gpu_kernels import RTOL, _spec_inputs, chain_kernel_case, close, words_from_seed

pytestmark = pytest.mark.gpu
ST = np.dtype([("fT", "f8"), ("fM", "f8"), ("t", "i4"), ("pad", "i4")])
NEGATE = 0x100                    # NLA_OBJ_NEGATE (include/nlopt_amd.h)
RCAP = 8192                       # NLA_ADV_RCAP (hip/dev_common.h): picks staged per segment by the advance kernel
MAXREL = {}                       # largest relative difference in f seen per launcher group (printed by the last test)


@pytest.fixture(scope="module")
def L():
    L = nlopt_amd.lib()
    assert nlopt_amd.device_count() > 0, "no HIP device: the product has no CPU fallback"
    return L


def zbuf(count, dtype=np.float64, fill=0):
    return DevBuf.from_array(np.full(count, fill, dtype))


def fclose(group, a, b, scale):
    """close() of test_gpu_kernels.py (same RTOL, same scale), recording the largest relative difference of the group"""
    a, b = np.asarray(a), np.asarray(b)
    if a.size:
        s = np.maximum(np.abs(b), scale)
        MAXREL[group] = max(MAXREL.get(group, 0.0), float(np.max(np.abs(a - b) / s)))
    return close(a, b, scale)


class Win:
    """a window of K stream blocks in the ring layout of test_advance_finish_commit_kernels: block b at ring entry b % ring, the
    window starting at block `first` (ring wrap and slot mask exercised); the oracle's digest of slot a in jn0 / pos0 / last0"""

    def __init__(self, obj, n, N, K, i0, seed, mask=255, align=2):
        self.P = P = O.port()
        self.obj, self.oid, self.n, self.N, self.K, self.i0, self.mask, self.nslot = obj, O.OBJ[obj], n, N, K, i0, mask, mask + 1
        self.ring = ring = K + 1
        self.first = first = 3 * ring + 2
        self.ld, self.lb, self.ub, self.X, self.w0, self.jn0, self.pos0, self.last0 = _spec_inputs(n, N, ring, seed, obj, align)
        ent = [(first + a) % ring for a in range(ring)]
        self.w = np.zeros(2 * n * ring, np.uint32)
        self.jn, self.pos, self.last = np.zeros(ring, np.int32), np.zeros(ring * n, np.int32), np.zeros(ring, np.int32)
        for a in range(ring):
            self.w[ent[a] * 2 * n:(ent[a] + 1) * 2 * n] = self.w0[a * 2 * n:(a + 1) * 2 * n]
            self.jn[ent[a]], self.last[ent[a]] = self.jn0[a], self.last0[a]
            self.pos[ent[a] * n:(ent[a] + 1) * n] = self.pos0[a * n:(a + 1) * n]
        self.q = [(first + a) & mask for a in range(K)]
        P.orc_k_advance_slot.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                         C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        P.orc_k_mutate.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        P.orc_k_eval.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]

    def rows(self, a):
        """the rows slot a picks, in pick order (crs.c:92,97,106,109: the best row is skipped)"""
        n, i0 = self.n, self.i0
        p = self.pos0[a * n:(a + 1) * n].astype(np.int64)
        r = p + (p >= i0)
        al = r[n - 1] + int(self.last0[a])
        r[n - 1] = al + (al == i0)
        return r

    def hazards(self, rng):
        """W[a-1] = a row sampled by slot a (slot a stops there or earlier); the best row in the list must be ignored"""
        K = self.K
        W = np.zeros(max(K, 1), np.int64)
        for a in range(1, K):
            W[a - 1] = self.rows(a)[int(rng.integers(0, self.n))]
        if K >= 3:
            W[K - 2] = self.i0
        return W, K - 1

    def advance(self, X, a, W, nun, t0, acc):
        n = self.n
        return self.P.orc_k_advance_slot(n, self.ld, X.ctypes.data, self.i0, int(self.jn0[a]), self.pos0[a * n:].ctypes.data, int(self.last0[a]),
                                         W.ctypes.data, nun, t0, self.lb.ctypes.data, self.ub.ctypes.data, acc.ctypes.data)

    def two_passes(self, W, nW):
        """the statement: pass 1 stopped by the hazard list, pass 2 with none; mutations and f of the finished points"""
        K, n, ld = self.K, self.n, self.ld
        acc, t1, t2 = np.zeros((K, ld)), np.zeros(K, np.int32), np.zeros(K, np.int32)
        for a in range(K):
            t1[a] = self.advance(self.X, a, W, min(a, nW), 0, acc[a])
        acc1 = acc.copy()
        for a in range(K):
            t2[a] = self.advance(self.X, a, W, 0, int(t1[a]), acc[a])
        assert np.all(t2 == n)
        TMr = np.zeros((K, ld))
        for a in range(K):
            self.P.orc_k_mutate(n, self.X[self.i0].ctypes.data, acc[a].ctypes.data, self.w0[(a + 1) * 2 * n:].ctypes.data, self.lb.ctypes.data,
                                self.ub.ctypes.data, TMr[a].ctypes.data)
        fTr, fMr = np.zeros(K), np.zeros(K)
        self.P.orc_k_eval(self.oid, n, ld, acc.ctypes.data, K, fTr.ctypes.data)
        self.P.orc_k_eval(self.oid, n, ld, TMr.ctypes.data, K, fMr.ctypes.data)
        return t1, acc1, acc, TMr, fTr, fMr

    def upload(self, X=None):
        X = self.X if X is None else X
        self.dX, self.dlb, self.dub, self.dw = DevBuf.from_array(X), DevBuf.from_array(self.lb), DevBuf.from_array(self.ub), DevBuf.from_array(self.w)
        self.dj, self.dp, self.dl = DevBuf.from_array(self.jn), DevBuf.from_array(self.pos), DevBuf.from_array(self.last)

    def slots(self, buf):
        return buf.to_array(np.float64, self.nslot * self.ld).reshape(self.nslot, self.ld)


def status_of(buf, K):
    return np.frombuffer(buf.to_array(np.uint8, ST.itemsize * K).tobytes(), dtype=ST)


class Outs:
    """one set of output buffers of a pass (zeroed: the kernels leave status.pad and the slots of other windows alone)"""

    def __init__(self, S, fill=0.0, ring_fill=0.0, nstatus=None):
        self.TX, self.TM = zbuf(S.nslot * S.ld, fill=fill), zbuf(S.nslot * S.ld, fill=fill)
        self.fT, self.fM = zbuf(S.nslot, fill=ring_fill), zbuf(S.nslot, fill=ring_fill)
        self.st = zbuf(ST.itemsize * (nstatus or S.K), np.uint8)
        self.t1, self.t2 = zbuf(S.K, np.int32, -1), zbuf(S.K, np.int32, -1)


# ---- A. lists as kernel arguments ----------------------------------------------------------------------------------------------------
A_CASES = [("sphere", 1, 4, 3, 2), ("sphere", 2, 9, 8, 4), ("rastrigin", 10, 13, 6, 12), ("griewank", 64, 70, 9, 33), ("levy", 65, 100, 7, 0),
           ("ackley", 127, 150, 6, 149), ("levy", 128, 140, 8, 17), ("rosenbrock", 129, 189, 5, 3), ("ackley", 257, 300, 6, 5),
           ("rosenbrock", 512, 520, 6, 3), ("griewank", 2048, 2060, 4, 77), ("rastrigin", 10, 40, 128, 7)]


@pytest.mark.parametrize("obj,n,N,K,i0", A_CASES)
def test_lists_as_kernel_arguments(L, obj, n, N, K, i0):
    """nla_k_crs_advance_args / nla_k_crs_finish_args / nla_k_crs_commit_args (W, t_in and the commit list as HOST arrays) in the two
    passes of test_advance_finish_commit_kernels: bit-exact TX / partial sums / t_out / TM, f within 1e-10, first-pass slots not
    recomputed; and, on the same inputs, bit-identical to the pointer forms (the same kernels).  n crosses every automatic tiling
    threshold (128, 512, 2048) and the vec2 condition (n even and >= 128); the last case is the limit K = 128, nW = 127."""
    S = Win(obj, n, N, K, i0, 31 + n)
    W, nW = S.hazards(np.random.default_rng(5 + n))
    assert K <= 128 and nW <= 128 and (K < 128 or nW == 127)
    t1r, acc1, TXr, TMr, fTr, fMr = S.two_passes(W, nW)
    scale = np.abs(np.concatenate([fTr, fMr])).mean()
    S.upload()
    dW = DevBuf.from_array(W)
    A, B = Outs(S), Outs(S)                       # A: the host-list forms; B: the pointer forms
    zero_t = np.zeros(K, np.int32)
    dzero_t = DevBuf.from_array(zero_t)
    q = S.q

    def pass_args(h_t_in, t_out, nw):
        assert L.nla_k_crs_advance_args(n, S.ld, S.dX.ptr, i0, S.dj.ptr, S.dp.ptr, S.dl.ptr, S.ring, S.first, K, W.ctypes.data, nw,
                                        h_t_in.ctypes.data, t_out.ptr, S.mask, S.dlb.ptr, S.dub.ptr, A.TX.ptr, 0, None) == 0
        assert L.nla_k_crs_finish_args(S.oid, n, S.ld, S.dX.ptr, i0, A.TX.ptr, A.TM.ptr, S.dw.ptr, S.ring, S.first, K, h_t_in.ctypes.data,
                                       t_out.ptr, S.mask, S.dlb.ptr, S.dub.ptr, A.fT.ptr, A.fM.ptr, A.st.ptr, None) == 0
        assert L.nla_stream_sync(None) == 0

    def pass_ptrs(t_in, t_out, nw):
        assert L.nla_k_crs_advance(n, S.ld, S.dX.ptr, i0, S.dj.ptr, S.dp.ptr, S.dl.ptr, S.ring, S.first, K, dW.ptr, nw, t_in.ptr, t_out.ptr,
                                   S.mask, S.dlb.ptr, S.dub.ptr, B.TX.ptr, 0, None) == 0
        assert L.nla_k_crs_finish(S.oid, n, S.ld, S.dX.ptr, i0, B.TX.ptr, B.TM.ptr, S.dw.ptr, S.ring, S.first, K, t_in.ptr, t_out.ptr, S.mask,
                                  S.dlb.ptr, S.dub.ptr, B.fT.ptr, B.fM.ptr, B.st.ptr, None) == 0
        assert L.nla_stream_sync(None) == 0

    def same_as_pointer_forms(ta, tb):
        assert np.array_equal(ta.to_array(np.int32, K), tb.to_array(np.int32, K))
        for x, y in ((A.TX, B.TX), (A.TM, B.TM)):
            assert S.slots(x).tobytes() == S.slots(y).tobytes()
        for x, y in ((A.fT, B.fT), (A.fM, B.fM)):
            assert x.to_array(np.float64, S.nslot).tobytes() == y.to_array(np.float64, S.nslot).tobytes()
        assert A.st.to_array(np.uint8, ST.itemsize * K).tobytes() == B.st.to_array(np.uint8, ST.itemsize * K).tobytes()

    pass_args(zero_t, A.t1, nW)
    pass_ptrs(dzero_t, B.t1, nW)
    st1 = status_of(A.st, K)
    t1 = A.t1.to_array(np.int32, K)
    assert np.array_equal(t1, t1r) and np.array_equal(st1["t"], t1r)
    TX1 = S.slots(A.TX)
    for a in range(K):
        if t1r[a] > 0:
            assert np.array_equal(TX1[q[a], :n], acc1[a, :n]), a        # partial sums are bit-exact too
    done1 = t1r == n
    assert done1[0] and (K < 3 or not done1.all())                     # the hazard list does stop slots
    assert fclose("A", st1["fT"][done1], fTr[done1], scale) and fclose("A", st1["fM"][done1], fMr[done1], scale)
    assert np.all(st1["fT"][~done1] == 0) and np.all(st1["fM"][~done1] == 0)
    same_as_pointer_forms(A.t1, B.t1)
    pass_args(t1, A.t2, 0)
    pass_ptrs(B.t1, B.t2, 0)
    st2 = status_of(A.st, K)
    assert np.all(A.t2.to_array(np.int32, K) == n) and np.all(st2["t"] == n)
    TX, TM = S.slots(A.TX)[q][:, :n], S.slots(A.TM)[q][:, :n]
    assert np.array_equal(TX, TXr[:, :n])          # bit-exact trial points (row order, no FMA)
    assert np.array_equal(TM, TMr[:, :n])          # bit-exact mutations
    assert fclose("A", st2["fT"], fTr, scale) and fclose("A", st2["fM"], fMr, scale)
    # slots finished in pass 1 keep their first-pass results (not recomputed)
    assert st2["fT"][done1].tobytes() == st1["fT"][done1].tobytes() and st2["fM"][done1].tobytes() == st1["fM"][done1].tobytes()
    same_as_pointer_forms(A.t2, B.t2)
    # ... and a third pass over the finished window writes no mutation again (TM of every slot replaced by a marker first)
    marker = np.full(S.nslot * S.ld, 7.25)
    assert L.nla_memcpy_h2d(A.TM.ptr, marker.ctypes.data, marker.nbytes, None) == 0
    full = np.full(K, n, np.int32)
    assert L.nla_k_crs_finish_args(S.oid, n, S.ld, S.dX.ptr, i0, A.TX.ptr, A.TM.ptr, S.dw.ptr, S.ring, S.first, K, full.ctypes.data, A.t2.ptr,
                                   S.mask, S.dlb.ptr, S.dub.ptr, A.fT.ptr, A.fM.ptr, A.st.ptr, None) == 0
    assert L.nla_stream_sync(None) == 0
    assert np.all(S.slots(A.TM) == 7.25) and status_of(A.st, K).tobytes() == st2.tobytes()
    # the commit: two candidates back into the population, lists as host arrays; the pointer form on a second population
    slot = np.array([q[0], q[K - 1]], np.int32)
    kind = np.array([1, 2], np.int32)
    rows = np.array([1 if i0 != 1 else 2, N - 1 if i0 != N - 1 else N - 2], np.int64)
    src = [0, K - 1]
    if K == 1:
        slot, kind, rows, src = slot[:1], kind[:1], rows[:1], src[:1]
    dX2 = DevBuf.from_array(S.X)
    ds, dk, dr = DevBuf.from_array(slot), DevBuf.from_array(kind), DevBuf.from_array(rows)
    # (A.TM holds the marker now; B.TM is bit-identical to what it held)
    assert L.nla_k_crs_commit_args(n, S.ld, S.dX.ptr, A.TX.ptr, B.TM.ptr, len(slot), slot.ctypes.data, kind.ctypes.data, rows.ctypes.data, None) == 0
    assert L.nla_k_crs_commit(n, S.ld, dX2.ptr, B.TX.ptr, B.TM.ptr, len(slot), ds.ptr, dk.ptr, dr.ptr, None) == 0
    assert L.nla_stream_sync(None) == 0
    Xe = S.X.copy()
    for a, k, r in zip(src, kind, rows):
        Xe[r, :n] = (TXr if k == 1 else TMr)[a, :n]
    X2 = S.dX.to_array(np.float64, N * S.ld).reshape(N, S.ld)
    assert np.array_equal(X2[:, :n], Xe[:, :n])
    assert X2.tobytes() == dX2.to_array(np.float64, N * S.ld).tobytes()


def test_list_launchers_refuse_more_than_128_entries(L):
    """K = 129 / nW = 129 / ncommit = 129: the lists would not fit the kernel arguments.  Every launcher returns non-zero before
    anything is launched (hip/crs_kernels.hip: the first statement of each), t_out and X stay as they were."""
    S = Win("sphere", 10, 40, 4, 7, 41)
    S.upload()
    big = 129
    o = Outs(S)
    t_out = zbuf(big, np.int32, -7)
    h_t, h_W = np.zeros(big, np.int32), np.arange(big, dtype=np.int64) % S.N
    for K, nw in ((big, 3), (4, big)):
        assert L.nla_k_crs_advance_args(S.n, S.ld, S.dX.ptr, S.i0, S.dj.ptr, S.dp.ptr, S.dl.ptr, S.ring, S.first, K, h_W.ctypes.data, nw,
                                        h_t.ctypes.data, t_out.ptr, S.mask, S.dlb.ptr, S.dub.ptr, o.TX.ptr, 0, None) != 0
        assert L.nla_k_crs_advance_commit_args(S.n, S.ld, S.dX.ptr, S.i0, S.dj.ptr, S.dp.ptr, S.dl.ptr, S.ring, S.first, K, h_W.ctypes.data, nw,
                                               h_t.ctypes.data, t_out.ptr, S.mask, S.dlb.ptr, S.dub.ptr, o.TX.ptr, o.TM.ptr, 0, None, None, None,
                                               0, None) != 0
    assert L.nla_k_crs_finish_args(S.oid, S.n, S.ld, S.dX.ptr, S.i0, o.TX.ptr, o.TM.ptr, S.dw.ptr, S.ring, S.first, big, h_t.ctypes.data, t_out.ptr,
                                   S.mask, S.dlb.ptr, S.dub.ptr, o.fT.ptr, o.fM.ptr, o.st.ptr, None) != 0
    slot, kind = np.zeros(big, np.int32), np.ones(big, np.int32)
    assert L.nla_k_crs_commit_args(S.n, S.ld, S.dX.ptr, o.TX.ptr, o.TM.ptr, big, slot.ctypes.data, kind.ctypes.data, h_W.ctypes.data, None) != 0
    assert L.nla_stream_sync(None) == 0
    assert np.all(t_out.to_array(np.int32, big) == -7)
    assert np.array_equal(S.dX.to_array(np.float64, S.N * S.ld).reshape(S.N, S.ld), S.X)
    assert not S.slots(o.TX).any() and not S.slots(o.TM).any()


# ---- B. the fused commit with forwarding ---------------------------------------------------------------------------------------------
B_CASES = [("rastrigin", 10, 11, 6, 10, 1, "plain"), ("griewank", 64, 66, 9, 33, 2, "best"), ("ackley", 257, 260, 7, 5, 16, "plain"),
           ("levy", 128, 131, 8, 17, 16, "in_W"), ("rosenbrock", 130, 132, 6, 3, 2, "jn"), ("ackley", 65, 67, 6, 66, 2, "last"),
           ("griewank", 512, 515, 5, 77, 16, "best"), ("sphere", 8200, 8203, 2, 5, 4, "far"),
           ("sphere", 8200, 8203, 2, 8000, 4, "far_in_W")]


@pytest.mark.parametrize("obj,n,N,K,i0,ncommit,what", B_CASES)
def test_fused_commit_forwards_every_read_of_a_committed_row(L, obj, n, N, K, i0, ncommit, what):
    """nla_k_crs_advance_commit_args: the commits staged by a previous window are copied by extra workgroups of the advance launch,
    and every read of such a row — a pick, or the best row a fresh slot starts from — is forwarded to the slot it is copied from.
    Against "the commit applied to a host copy of X, then the whole-row statement": X afterwards, the window's TX (partial sums of
    stopped slots included) and t_out bit for bit; the source slots unchanged.  N is barely above n, so nearly every row is picked
    by every slot.  Half of the slots resume a sum begun on the old population (they must not re-read the best row), the others
    are fresh.  what: best = the best row is committed; in_W = a committed row is also a hazard (the plan searches by row number
    before forwarding: the slot stops there); jn / last = the pick subtracted with weight n/2 / the last pick (formed from
    last_ring) is committed; far = n > 8192 with committed rows at pick positions >= 8192 of a fresh slot (the kernel's second
    staging loop); far_in_W = there, one of them is also a hazard: the plan finds it in the pick list in memory, behind the staged
    picks, and the slot stops inside the second segment.  Each case asserts from the oracle's pick lists that its situation occurs."""
    S = Win(obj, n, N, K, i0, 77 + n)
    ld, X = S.ld, S.X
    rng = np.random.default_rng(11 + n)
    rows_of = [S.rows(a) for a in range(K)]
    # a first pass on the old population leaves partial sums; odd slots resume them, even slots are fresh
    W1, nW1 = S.hazards(rng)
    acc = np.full((K, ld), 3.5)                   # (a fresh slot that cannot advance leaves TX as it is: the same marker on the device)
    t_in = np.zeros(K, np.int32)
    for a in (range(1, K, 2) if what != "far_in_W" else ()):       # (far_in_W: every slot fresh)
        part = np.zeros(ld)
        t = S.advance(X, a, W1, min(a, nW1), 0, part)
        if 0 < t < n:
            t_in[a], acc[a] = t, part
    # the rows the case is about, then random other rows up to ncommit; never the best row unless the case says so
    need, W2, nW2, a_star, t_star = [], np.zeros(1, np.int64), 0, K - 1, -1
    if what == "best":
        need = [i0]
    elif what == "in_W":
        t_star = min(n - 1, int(t_in[a_star]) + max(2, (n - int(t_in[a_star])) // 2))
        need = [int(rows_of[a_star][t_star]), int(rows_of[a_star][t_in[a_star]])]
        W2[0], nW2 = need[0], 1
    elif what == "jn":
        need = [int(rows_of[0][S.jn0[0]])]
    elif what == "last":
        need = [int(rows_of[0][n - 1])]
    elif what == "far":
        need = [int(r) for r in rows_of[0][RCAP:RCAP + ncommit]]
    elif what == "far_in_W":
        t_star = RCAP + 3
        need = [int(rows_of[a_star][t_star])] + [int(r) for r in rows_of[a_star][RCAP:RCAP + 2]]
        W2[0], nW2 = need[0], 1
    need = list(dict.fromkeys(need))[:ncommit]
    others = [int(r) for r in rng.permutation(N) if r != i0 and r not in need]
    c_row = np.array(need + others[:ncommit - len(need)], np.int64)
    assert len(c_row) == ncommit and len(set(c_row.tolist())) == ncommit
    c_kind = np.array([1 + c % 2 for c in range(ncommit)], np.int32)
    c_slot = np.array([(S.first + K + 3 + c) & S.mask for c in range(ncommit)], np.int32)
    assert not set(c_slot.tolist()) & set(S.q)
    TX0, TM0 = np.full((S.nslot, ld), 3.5), np.full((S.nslot, ld), -3.5)
    for a in range(K):
        TX0[S.q[a]] = acc[a]
    for s_, k_ in zip(c_slot, c_kind):
        (TX0 if k_ == 1 else TM0)[s_, :n] = rng.uniform(S.lb, S.ub)
        (TX0 if k_ == 1 else TM0)[s_, n:] = 0
    # the device gets the old population; the host copy is committed in place (one copy of a large X less)
    S.upload()
    old_rows = X[c_row].copy()
    for s_, k_, r_ in zip(c_slot, c_kind, c_row):
        X[r_, :n] = (TX0 if k_ == 1 else TM0)[s_, :n]
    assert all(not np.array_equal(X[r_, :n], o_[:n]) for r_, o_ in zip(c_row, old_rows))
    t_out = np.zeros(K, np.int32)
    for a in range(K):
        t_out[a] = S.advance(X, a, W2, min(a, nW2), int(t_in[a]), acc[a])
    # the situation the case is named after does occur
    cset = set(c_row.tolist())
    hits = [[t for t in range(int(t_in[a]), int(t_out[a])) if int(rows_of[a][t]) in cset] for a in range(K)]
    assert sum(len(h) for h in hits) > 0
    fresh = [a for a in range(K) if t_in[a] == 0 and t_out[a] > 0]
    resumed = [a for a in range(K) if 0 < t_in[a] < n and t_out[a] > t_in[a]]
    assert fresh and (K < 4 or resumed)
    if what == "best":
        assert i0 in cset and fresh and resumed
    elif what == "in_W":
        assert t_out[a_star] == t_star < n and int(rows_of[a_star][t_star]) in cset and hits[a_star]
    elif what == "jn":
        assert int(S.jn0[0]) in hits[0]
    elif what == "last":
        assert n - 1 in hits[0]
    elif what == "far":
        assert n > RCAP and t_in[0] == 0 and max(hits[0]) >= RCAP
    elif what == "far_in_W":
        assert t_in[a_star] == 0 and t_out[a_star] == t_star >= RCAP and max(hits[a_star]) >= RCAP and t_out[0] == n
    if what not in ("in_W", "far_in_W"):
        assert np.all(t_out == n)
    dTX, dTM, dt = DevBuf.from_array(TX0), DevBuf.from_array(TM0), zbuf(K, np.int32, -1)
    assert L.nla_k_crs_advance_commit_args(n, ld, S.dX.ptr, i0, S.dj.ptr, S.dp.ptr, S.dl.ptr, S.ring, S.first, K, W2.ctypes.data, nW2,
                                           t_in.ctypes.data, dt.ptr, S.mask, S.dlb.ptr, S.dub.ptr, dTX.ptr, dTM.ptr, ncommit, c_slot.ctypes.data,
                                           c_kind.ctypes.data, c_row.ctypes.data, 0, None) == 0
    assert L.nla_stream_sync(None) == 0
    assert np.array_equal(dt.to_array(np.int32, K), t_out)
    Xd = S.dX.to_array(np.float64, N * ld).reshape(N, ld)
    assert np.array_equal(Xd, X)                  # the committed copy; rows not committed untouched
    del Xd
    TX, TM = S.slots(dTX), S.slots(dTM)
    for a in range(K):
        assert np.array_equal(TX[S.q[a], :n], acc[a, :n]), (a, int(t_in[a]), int(t_out[a]))
    outside = np.setdiff1d(np.arange(S.nslot), S.q)
    assert np.array_equal(TX[outside], TX0[outside]) and np.array_equal(TM, TM0)          # the source slots (and every other) unchanged


def test_fused_commit_refuses_more_than_16_commits(L):
    """ncommit = 17 and ncommit < 0: non-zero return before anything is launched, X untouched"""
    S = Win("sphere", 10, 13, 4, 7, 43)
    S.upload()
    o = Outs(S)
    t_in, W = np.zeros(4, np.int32), np.zeros(1, np.int64)
    slot, kind, row = np.arange(40, 57, dtype=np.int32), np.ones(17, np.int32), np.arange(17, dtype=np.int64) % S.N
    for nc in (17, -1):
        assert L.nla_k_crs_advance_commit_args(S.n, S.ld, S.dX.ptr, S.i0, S.dj.ptr, S.dp.ptr, S.dl.ptr, S.ring, S.first, 4, W.ctypes.data, 0,
                                               t_in.ctypes.data, o.t1.ptr, S.mask, S.dlb.ptr, S.dub.ptr, o.TX.ptr, o.TM.ptr, nc, slot.ctypes.data,
                                               kind.ctypes.data, row.ctypes.data, 0, None) != 0
    assert L.nla_stream_sync(None) == 0
    assert np.array_equal(S.dX.to_array(np.float64, S.N * S.ld).reshape(S.N, S.ld), S.X)
    assert np.all(o.t1.to_array(np.int32, 4) == -1)


# ---- C. the doorbell; finish without a built-in objective ------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 128])
def test_finish_with_doorbell(L, K):
    """nla_k_crs_finish_args_bell: status and bell in pinned host memory, bell_count a zeroed device word.  After the stream is
    synchronised *bell == seq, the count is back at zero (reset by the last of the 2K workgroups) and the K records are
    nla_k_crs_finish_args's bit for bit; a second launch on the same words with seq + 1 tests the reset."""
    n, N, i0 = 10, 40, 7
    S = Win("rastrigin", n, N, K, i0, 51 + K)
    W, nW = S.hazards(np.random.default_rng(K))
    t1r = S.two_passes(W, nW)[0]
    S.upload()
    A, B = Outs(S), Outs(S)
    pinned = L.nla_host_malloc(ST.itemsize * K + 8)
    assert pinned
    try:
        C.memset(pinned, 0, ST.itemsize * K + 8)
        bell = pinned + ST.itemsize * K
        count = zbuf(1, np.uint32)
        seq = 41
        t_in = np.zeros(K, np.int32)
        for p, (t_out, nw) in enumerate(((A.t1, nW), (A.t2, 0))):
            assert L.nla_k_crs_advance_args(n, S.ld, S.dX.ptr, i0, S.dj.ptr, S.dp.ptr, S.dl.ptr, S.ring, S.first, K, W.ctypes.data, nw,
                                            t_in.ctypes.data, t_out.ptr, S.mask, S.dlb.ptr, S.dub.ptr, A.TX.ptr, 0, None) == 0
            assert L.nla_k_crs_finish_args(S.oid, n, S.ld, S.dX.ptr, i0, A.TX.ptr, A.TM.ptr, S.dw.ptr, S.ring, S.first, K, t_in.ctypes.data, t_out.ptr,
                                           S.mask, S.dlb.ptr, S.dub.ptr, A.fT.ptr, A.fM.ptr, A.st.ptr, None) == 0
            assert L.nla_k_crs_finish_args_bell(S.oid, n, S.ld, S.dX.ptr, i0, A.TX.ptr, B.TM.ptr, S.dw.ptr, S.ring, S.first, K, t_in.ctypes.data,
                                                t_out.ptr, S.mask, S.dlb.ptr, S.dub.ptr, B.fT.ptr, B.fM.ptr, pinned, count.ptr, bell, seq + p,
                                                None) == 0
            assert L.nla_stream_sync(None) == 0
            assert C.c_uint32.from_address(bell).value == seq + p
            assert count.to_array(np.uint32, 1)[0] == 0
            rec = np.frombuffer(C.string_at(pinned, ST.itemsize * K), dtype=ST)
            assert rec.tobytes() == A.st.to_array(np.uint8, ST.itemsize * K).tobytes()
            assert np.array_equal(rec["t"], t1r if p == 0 else np.full(K, n))
            assert S.slots(A.TM).tobytes() == S.slots(B.TM).tobytes()
            assert A.fT.to_array(np.float64, S.nslot).tobytes() == B.fT.to_array(np.float64, S.nslot).tobytes()
            t_in = t_out.to_array(np.int32, K)
        # refused without a bell or a count word: nothing launched, the bell keeps its value
        for bc, b in ((None, bell), (count.ptr, None)):
            assert L.nla_k_crs_finish_args_bell(S.oid, n, S.ld, S.dX.ptr, i0, A.TX.ptr, B.TM.ptr, S.dw.ptr, S.ring, S.first, K, t_in.ctypes.data,
                                                A.t2.ptr, S.mask, S.dlb.ptr, S.dub.ptr, B.fT.ptr, B.fM.ptr, pinned, bc, b, seq + 9, None) != 0
        assert L.nla_stream_sync(None) == 0
        assert C.c_uint32.from_address(bell).value == seq + 1 and count.to_array(np.uint32, 1)[0] == 0
    finally:
        L.nla_host_free(pinned)


@pytest.mark.parametrize("obj,n,N,K,i0", [("rastrigin", 10, 30, 7, 3), ("ackley", 257, 300, 6, 5), ("griewank", 1, 5, 4, 0)])
def test_finish_without_a_builtin_objective_and_negated(L, obj, n, N, K, i0):
    """nla_k_crs_finish with obj = -1 (host-callback mode: status.t only, no evaluation, no mutation), obj = -2 (user-kernel mode: the
    mutation only) and obj | NLA_OBJ_NEGATE (the exact negatives of the plain launch's f).  TM, fT_ring and fM_ring carry markers."""
    S = Win(obj, n, N, K, i0, 61 + n)
    W, nW = S.hazards(np.random.default_rng(2 + n))
    t1r, acc1, TXr, TMr, fTr, fMr = S.two_passes(W, nW)
    scale = np.abs(np.concatenate([fTr, fMr])).mean()
    S.upload()
    dW = DevBuf.from_array(W)
    H, U, Pl, Ng = (Outs(S, fill=7.25, ring_fill=-3.5) for _ in range(4))      # host-callback, user-kernel, plain, negated
    TX = zbuf(S.nslot * S.ld)
    t0 = zbuf(K, np.int32)
    ts = [t0, zbuf(K, np.int32, -1), zbuf(K, np.int32, -1)]
    q = S.q
    done_before = np.zeros(K, bool)
    for p, nw in enumerate((nW, 0)):
        t_in, t_out = ts[p], ts[p + 1]
        assert L.nla_k_crs_advance(n, S.ld, S.dX.ptr, i0, S.dj.ptr, S.dp.ptr, S.dl.ptr, S.ring, S.first, K, dW.ptr, nw, t_in.ptr, t_out.ptr,
                                   S.mask, S.dlb.ptr, S.dub.ptr, TX.ptr, 0, None) == 0
        for o, oid in ((H, -1), (U, -2), (Pl, S.oid), (Ng, S.oid | NEGATE)):
            assert L.nla_k_crs_finish(oid, n, S.ld, S.dX.ptr, i0, TX.ptr, o.TM.ptr, S.dw.ptr, S.ring, S.first, K, t_in.ptr, t_out.ptr, S.mask,
                                      S.dlb.ptr, S.dub.ptr, o.fT.ptr, o.fM.ptr, o.st.ptr, None) == 0
        assert L.nla_stream_sync(None) == 0
        tr = t1r if p == 0 else np.full(K, n, np.int32)
        done = tr == n
        # obj = -1
        st = status_of(H.st, K)
        assert np.array_equal(st["t"], tr) and np.all(st["fT"] == 0) and np.all(st["fM"] == 0)
        assert np.all(S.slots(H.TM) == 7.25)
        assert np.all(H.fT.to_array(np.float64, S.nslot) == -3.5) and np.all(H.fM.to_array(np.float64, S.nslot) == -3.5)
        # obj = -2
        st = status_of(U.st, K)
        assert np.array_equal(st["t"], tr) and np.all(st["fT"] == 0) and np.all(st["fM"] == 0)
        TMu = S.slots(U.TM)
        want = np.full((S.nslot, S.ld), 7.25)
        for a in range(K):
            if done[a]:
                want[q[a], :n] = TMr[a, :n]
        assert np.array_equal(TMu[:, :n], want[:, :n])
        assert np.all(U.fT.to_array(np.float64, S.nslot) == -3.5) and np.all(U.fM.to_array(np.float64, S.nslot) == -3.5)
        if p == 0:          # a marker in the mutation of a slot finished in pass 1: pass 2 must not form it again
            row = np.full(S.ld, 9.75)
            assert L.nla_memcpy_h2d(U.TM.ptr + 8 * S.ld * q[0], row.ctypes.data, row.nbytes, None) == 0
            TMr_keep = TMr[0].copy()
            TMr[0, :n] = 9.75
        # negated against plain
        sp, sn = status_of(Pl.st, K), status_of(Ng.st, K)
        assert fclose("C", sp["fT"][done], fTr[done], scale) and fclose("C", sp["fM"][done], fMr[done], scale)
        assert np.array_equal(-sp["fT"][done], sn["fT"][done]) and np.array_equal(-sp["fM"][done], sn["fM"][done])
        assert np.all(np.signbit(sn["fT"][done]) != np.signbit(sp["fT"][done]))
        assert np.array_equal(S.slots(Pl.TM)[q][done], S.slots(Ng.TM)[q][done])
        done_before = done
    TMr[0] = TMr_keep
    assert done_before.all()


# ---- D. the production form of the window launch ---------------------------------------------------------------------------------------
D_CASES = [("rastrigin", 10, 11, 9, 10), ("griewank", 64, 70, 60, 33), ("ackley", 257, 600, 40, 599), ("ackley", 300, 320, 30, 5),
           ("levy", 128, 140, 128, 17)]


@pytest.mark.parametrize("lists", ["host", "dev"])
@pytest.mark.parametrize("obj,n,N,K,i0", D_CASES)
def test_window_launch_as_the_engine_issues_it(L, obj, n, N, K, i0, lists):
    """nla_k_crs_commit_zero + nla_k_crs_chain_lean(w_on_host = 1, ctrl_is_zero = 1) with pinned outputs: chain_kernel_case of
    test_gpu_kernels.py in its lean mode (the clearing is asserted before the window is launched), commit lists as host / device arrays"""
    MAXREL["D"] = max(MAXREL.get("D", 0.0), chain_kernel_case(L, obj, n, N, K, i0, lean=lists))


def test_window_launchers_refuse(L):
    """nla_k_crs_commit_zero: ncommit = 0, zero_bytes not a multiple of 4, 129 commits as kernel arguments; nla_k_crs_chain_lean: 129
    hazard rows as kernel arguments.  hip/crs_kernels.hip, hip/crs_chain.hip: each returns before its launch; nothing is written."""
    n, N, K, i0 = 10, 200, 4, 3
    ld = 16
    X = np.random.default_rng(1).uniform(-1, 1, (N, ld))
    dX, dTX, dTM = DevBuf.from_array(X), DevBuf.from_array(np.zeros(512 * ld), uncached=True), DevBuf.from_array(np.zeros(512 * ld), uncached=True)
    cb = L.nla_crs_chain_ctrl_bytes(256, 256)
    blk = np.full(cb, 0xA5, np.uint8)
    dctrl = DevBuf.from_array(blk, uncached=True)
    slot, kind, row = np.zeros(129, np.int32), np.ones(129, np.int32), np.arange(129, dtype=np.int64)
    for ncommit, zb, host in ((0, 64, 1), (0, 64, 0), (1, 62, 1), (1, 61, 0), (129, 64, 1)):
        assert L.nla_k_crs_commit_zero(n, ld, dX.ptr, dTX.ptr, dTM.ptr, ncommit, slot.ctypes.data, kind.ctypes.data, row.ctypes.data, host,
                                       dctrl.ptr + 4, zb, None) != 0
    W, Wf = np.arange(129, dtype=np.int64), np.linspace(9, 1, 129)
    lb, ub = DevBuf.from_array(np.full(ld, -1.0)), DevBuf.from_array(np.full(ld, 1.0))
    ring = 2 * K + 3
    dj, dp, dl, dw = zbuf(ring, np.int32), zbuf(ring * n, np.int32), zbuf(ring, np.int32), zbuf(2 * n * ring, np.uint32)
    dst, dcnt, drec = zbuf(ST.itemsize * K, np.uint8), zbuf(K, np.uint32), zbuf(K * 48, np.uint32)
    assert L.nla_k_crs_chain_lean(0, n, ld, dX.ptr, i0, -1.0, dj.ptr, dp.ptr, dl.ptr, dw.ptr, ring, 0, K, W.ctypes.data, Wf.ctypes.data, 129, 1, 511,
                                  lb.ptr, ub.ptr, dTX.ptr, dTM.ptr, dctrl.ptr, 0, dst.ptr, dcnt.ptr, drec.ptr, 48, 1, None) != 0
    assert L.nla_stream_sync(None) == 0
    assert np.array_equal(dctrl.to_array(np.uint8, cb), blk)
    assert np.array_equal(dX.to_array(np.float64, N * ld).reshape(N, ld), X)
    assert not dst.to_array(np.uint8, ST.itemsize * K).any()


# ---- E. the single mutation in place ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_mutate_in_place(L, n):
    """nla_k_crs_mutate (host-callback mode, crs.c:139-146) in place, bit for bit against orc_k_mutate; bounds so narrow that the
    reference clamps at both ends, one coordinate with lb == ub.  (n = 1 has one coordinate: three launches, one for each.)"""
    P = O.port()
    P.orc_k_mutate.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    rng = np.random.default_rng(300 + n)
    n_hi = n_lo = n_fix = 0
    for launch in range(3 if n == 1 else 1):
        w = words_from_seed(900 + n + launch, 2 * n)
        best, p = rng.uniform(-5, 5, n), rng.uniform(-5, 5, n)
        lb, ub = best - rng.uniform(0, 0.5, n), best + rng.uniform(0, 0.5, n)
        wv = ((w[0::2] >> 5) * 67108864.0 + (w[1::2] >> 6)) * (1.0 / 9007199254740992.0)
        v = best * (1 + wv) - wv * p
        if n == 1:          # one coordinate: make it clamp above, below, or be fixed
            if launch == 0:
                ub = v - 0.25
                lb = ub - 1
            elif launch == 1:
                lb = v + 0.25
                ub = lb + 1
            else:
                lb = ub = best.copy()
        else:
            lb[n // 2] = ub[n // 2] = best[n // 2] + 0.125
        ref = np.zeros(n)
        P.orc_k_mutate(n, best.ctypes.data, p.ctypes.data, w.ctypes.data, lb.ctypes.data, ub.ctypes.data, ref.ctypes.data)
        n_hi += int(np.sum((v > ub) & (ref == ub) & (lb < ub)))
        n_lo += int(np.sum((v < lb) & (ref == lb) & (lb < ub)))
        n_fix += int(np.sum((lb == ub) & (ref == lb)))
        assert np.any((ref > lb) & (ref < ub)) or n == 1
        db, dp, dw, dlb, dub = (DevBuf.from_array(x) for x in (best, p, w, lb, ub))
        assert L.nla_k_crs_mutate(n, db.ptr, dp.ptr, dw.ptr, dlb.ptr, dub.ptr, None) == 0
        assert L.nla_stream_sync(None) == 0
        assert np.array_equal(dp.to_array(np.float64, n), ref)
        assert np.array_equal(db.to_array(np.float64, n), best)
    assert n_hi >= 1 and n_lo >= 1 and n_fix >= 1


# ---- F. the column-sharded pass, the ranks one after the other on one device -------------------------------------------------------------
def shard_layout(n, world):
    """crs_engine.c: colper = ceil(n / world), rank r holds columns [c0, c0 + nc), rows ld apart; the gather runs over ncol columns
    (one zero pad column more when nc is odd: coordinate pairs)"""
    colper = (n + world - 1) // world
    out = []
    for r in range(world):
        c0 = r * colper
        nc = min(colper, n - c0)
        ld = (nc + 15) & ~15
        out.append((c0, nc, ld, nc + 1 if (nc % 2 and ld % 2 == 0) else nc))
    return colper, out


F_CASES = [(2, 259, "ackley"), (3, 11, "rastrigin"), (4, 517, "griewank"), (2, 5, "levy")]


def test_shard_cases_cover_the_layouts():
    """(no device needed, but it belongs to the cases below) the last rank's slice is shorter than colper, some nc is odd, and one
    slice runs the vec2 kernel (ncol even and >= 128) over its zero pad column"""
    short = odd = vec2_pad = False
    for world, n, _ in F_CASES:
        colper, lay = shard_layout(n, world)
        assert sum(nc for _, nc, _, _ in lay) == n and all(nc >= 1 for _, nc, _, _ in lay)
        short |= lay[-1][1] < colper
        odd |= any(nc % 2 for _, nc, _, _ in lay)
        vec2_pad |= any(ncol > nc and ncol >= 128 and ncol % 2 == 0 for _, nc, _, ncol in lay)
    assert short and odd and vec2_pad


@pytest.mark.parametrize("world,n,obj", F_CASES)
def test_shard_init_rows(L, world, n, obj):
    """nla_k_crs_sh_init_rows: the slice is columns [c0, c0 + nc) of the whole orc_k_init_rows result, pad columns zero, written at
    row_first = 3 (the rows in front untouched)"""
    P = O.port()
    nrows, row_first = 37, 3
    lo, hi = nlopt_amd.objective_box(obj)
    lb, ub = np.full(n, lo), np.linspace(hi * 0.5, hi, n)
    w = words_from_seed(99 + n, 2 * n * nrows)
    Xr = np.zeros((nrows, n))
    P.orc_k_init_rows.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    P.orc_k_init_rows(n, n, lb.ctypes.data, ub.ctypes.data, w.ctypes.data, nrows, Xr.ctypes.data)
    dw = DevBuf.from_array(w)
    colper, lay = shard_layout(n, world)
    for c0, nc, ld, _ in lay:
        lbs, ubs = np.zeros(ld), np.zeros(ld)
        lbs[:nc], ubs[:nc] = lb[c0:c0 + nc], ub[c0:c0 + nc]
        dlb, dub = DevBuf.from_array(lbs), DevBuf.from_array(ubs)
        dX = zbuf((nrows + row_first) * ld, fill=-9.0)
        assert L.nla_k_crs_sh_init_rows(n, c0, nc, ld, dlb.ptr, dub.ptr, dw.ptr, row_first, nrows, dX.ptr, None) == 0
        assert L.nla_stream_sync(None) == 0
        X = dX.to_array(np.float64, (nrows + row_first) * ld).reshape(nrows + row_first, ld)
        assert np.all(X[:row_first] == -9.0)
        assert np.array_equal(X[row_first:, :nc], Xr[:, c0:c0 + nc]), c0
        assert not X[row_first:, nc:].any()


@pytest.mark.parametrize("world,n,obj", F_CASES)
def test_shard_pass(L, world, n, obj):
    """one conservative pass of a column-sharded run, twice (the first stopped by a hazard list), every rank on this device in turn:
    nla_k_crs_advance_cols, nla_k_crs_sh_mutate_pack, then nla_k_crs_sh_eval on the concatenation of the ranks' SEND blocks.
    Expectations are the whole-row statements sliced; on the device the f values of nla_k_crs_sh_eval are also bit-identical to
    nla_k_crs_finish's for the same points on a whole-row population — what crs_shard.hip and the multi-process tests rest on."""
    K, i0 = 7, 4
    N = n + 20
    S = Win(obj, n, N, K, i0, 91 + n, mask=63, align=16)
    W, nW = S.hazards(np.random.default_rng(8 + n))
    t1r, acc1, TXr, TMr, fTr, fMr = S.two_passes(W, nW)
    assert (t1r == n).any() and (t1r < n).any()
    scale = np.abs(np.concatenate([fTr, fMr])).mean()
    colper, lay = shard_layout(n, world)
    q, nslot = S.q, S.nslot
    S.upload()                                   # the whole-row population: nla_k_crs_finish's side of the comparison
    dW = DevBuf.from_array(W)
    rs = 2 * K * colper + 2                       # a rank's block of the all-gather
    RECV = [np.zeros(world * rs), np.zeros(world * rs)]
    flags = [[(1 if (world >= 3 and r == 1) else 0, 0) for r in range(world)],
             [(2 if r == world - 1 else 0, 1 if r == 0 else 0) for r in range(world)]]
    dzero = zbuf(K, np.int32)
    combos = list(itertools.product((0, 1, 2), (0, 1)))
    for r, (c0, nc, ld, ncol) in enumerate(lay):
        Xs, lbs, ubs = np.zeros((N, ld)), np.zeros(ld), np.zeros(ld)
        Xs[:, :nc], lbs[:nc], ubs[:nc] = S.X[:, c0:c0 + nc], S.lb[c0:c0 + nc], S.ub[c0:c0 + nc]
        dXs, dlb, dub = DevBuf.from_array(Xs), DevBuf.from_array(lbs), DevBuf.from_array(ubs)
        dTX, dTM = zbuf(nslot * ld), zbuf(nslot * ld, fill=7.25)
        ts = [dzero, zbuf(K, np.int32, -1), zbuf(K, np.int32, -1)]
        for p, nw in enumerate((nW, 0)):
            t_in, t_out = ts[p], ts[p + 1]
            tin_r = np.zeros(K, np.int32) if p == 0 else t1r
            tr = t1r if p == 0 else np.full(K, n, np.int32)
            newly = (tr == n) & (tin_r != n)
            assert L.nla_k_crs_advance_cols(n, ncol, ld, dXs.ptr, i0, S.dj.ptr, S.dp.ptr, S.dl.ptr, S.ring, S.first, K, dW.ptr, nw, t_in.ptr,
                                            t_out.ptr, S.mask, dlb.ptr, dub.ptr, dTX.ptr, 0, None) == 0
            dSEND = zbuf(rs, fill=-6.5)
            ff, ft = flags[p][r]
            assert L.nla_k_crs_sh_mutate_pack(n, c0, nc, ld, colper, dXs.ptr, i0, dTX.ptr, dTM.ptr, S.dw.ptr, S.ring, S.first, K, t_in.ptr,
                                              t_out.ptr, S.mask, dlb.ptr, dub.ptr, dSEND.ptr, ff, ft, None) == 0
            assert L.nla_stream_sync(None) == 0
            assert np.array_equal(t_out.to_array(np.int32, K), tr), r             # identical on every rank: the statement's
            TX = dTX.to_array(np.float64, nslot * ld).reshape(nslot, ld)
            TM = dTM.to_array(np.float64, nslot * ld).reshape(nslot, ld)
            ref = acc1 if p == 0 else TXr
            for a in range(K):
                if tr[a] > 0:
                    assert np.array_equal(TX[q[a], :nc], ref[a, c0:c0 + nc]), (r, p, a)     # partial sums included
                assert not TX[q[a], nc:].any()                                             # the pad columns stay zero
            SEND = dSEND.to_array(np.float64, rs)
            want = np.full(rs, -6.5)
            for a in range(K):
                if newly[a]:
                    want[2 * a * colper:2 * a * colper + nc] = TXr[a, c0:c0 + nc]
                    want[(2 * a + 1) * colper:(2 * a + 1) * colper + nc] = TMr[a, c0:c0 + nc]
                    assert np.array_equal(TM[q[a], :nc], TMr[a, c0:c0 + nc]) and not TM[q[a], nc:].any(), (r, p, a)
                elif tin_r[a] != n:
                    assert np.all(TM[q[a]] == 7.25), (r, p, a)
            want[rs - 2], want[rs - 1] = ff, ft
            assert np.array_equal(SEND, want), (r, p)
            RECV[p][r * rs:(r + 1) * rs] = SEND
        # every value of the two stop flags, on a pass that completes nothing: the flags and nothing else
        for ff, ft in combos:
            dSEND = zbuf(rs, fill=-6.5)
            assert L.nla_k_crs_sh_mutate_pack(n, c0, nc, ld, colper, dXs.ptr, i0, dTX.ptr, dTM.ptr, S.dw.ptr, S.ring, S.first, K, ts[2].ptr,
                                              ts[2].ptr, S.mask, dlb.ptr, dub.ptr, dSEND.ptr, ff, ft, None) == 0
            assert L.nla_stream_sync(None) == 0
            want = np.full(rs, -6.5)
            want[rs - 2], want[rs - 1] = ff, ft
            assert np.array_equal(dSEND.to_array(np.float64, rs), want)
        # a slice wider than colper is refused before the launch
        dSEND = zbuf(rs + 2 * K, fill=-6.5)
        assert L.nla_k_crs_sh_mutate_pack(n, c0, nc, ld, nc - 1, dXs.ptr, i0, dTX.ptr, dTM.ptr, S.dw.ptr, S.ring, S.first, K, ts[1].ptr,
                                          ts[2].ptr, S.mask, dlb.ptr, dub.ptr, dSEND.ptr, 0, 0, None) != 0
        assert L.nla_stream_sync(None) == 0
        assert np.all(dSEND.to_array(np.float64, rs + 2 * K) == -6.5)
    # the evaluation of the gathered candidates, and nla_k_crs_finish on the assembled points of a whole-row population
    E, Fi = Outs(S, nstatus=K + 1), Outs(S)
    TXw = zbuf(nslot * S.ld)
    t_ins, t_outs = [np.zeros(K, np.int32), t1r], [t1r, np.full(K, n, np.int32)]
    prev = None
    for p in range(2):
        dti, dto = DevBuf.from_array(t_ins[p]), DevBuf.from_array(t_outs[p])
        dR = DevBuf.from_array(RECV[p])
        whole = np.zeros((nslot, S.ld))
        whole[q] = acc1 if p == 0 else TXr
        assert L.nla_memcpy_h2d(TXw.ptr, whole.ctypes.data, whole.nbytes, None) == 0
        assert L.nla_k_crs_sh_eval(S.oid, n, colper, S.first, K, dti.ptr, dto.ptr, S.mask, dR.ptr, world, E.fT.ptr, E.fM.ptr, E.st.ptr, None) == 0
        assert L.nla_k_crs_finish(S.oid, n, S.ld, S.dX.ptr, i0, TXw.ptr, Fi.TM.ptr, S.dw.ptr, S.ring, S.first, K, dti.ptr, dto.ptr, S.mask,
                                  S.dlb.ptr, S.dub.ptr, Fi.fT.ptr, Fi.fM.ptr, Fi.st.ptr, None) == 0
        assert L.nla_stream_sync(None) == 0
        st, sf = status_of(E.st, K + 1), status_of(Fi.st, K)
        done = t_outs[p] == n
        assert np.array_equal(st["t"][:K], t_outs[p])
        assert fclose("F", st["fT"][:K][done], fTr[done], scale) and fclose("F", st["fM"][:K][done], fMr[done], scale)
        assert np.all(st["fT"][:K][~done] == 0) and np.all(st["fM"][:K][~done] == 0)                 # unfinished: 0
        assert st[:K].tobytes() == sf.tobytes()                                                         # bit-identical to the whole-row finish
        assert E.fT.to_array(np.float64, nslot).tobytes() == Fi.fT.to_array(np.float64, nslot).tobytes()
        assert E.fM.to_array(np.float64, nslot).tobytes() == Fi.fM.to_array(np.float64, nslot).tobytes()
        assert np.array_equal(S.slots(Fi.TM)[q][done][:, :n], TMr[done][:, :n])                       # (and its mutation is the ranks')
        if prev is not None:                     # complete before the pass: the ring values, i.e. the first pass's
            was = t_ins[p] == n
            assert was.any() and st["fT"][:K][was].tobytes() == prev["fT"][:K][was].tobytes()
            assert st["fM"][:K][was].tobytes() == prev["fM"][:K][was].tobytes()
        f0 = 1.0 if any(f for f, _ in flags[p]) else 0.0
        f1 = 1.0 if any(t for _, t in flags[p]) else 0.0
        failed = 1 if any(f == 2 for f, _ in flags[p]) else 0
        assert (st["fT"][K], st["fM"][K], st["t"][K]) == (f0, f1, failed), p
        prev = st.copy()
    assert prev["t"][K] == 1


@pytest.mark.parametrize("world,n", [(w, n) for w, n, _ in F_CASES])
def test_shard_commit(L, world, n):
    """nla_k_crs_commit_sh: rows of the slice from whole points at stride ldf, the control block cleared, xbest refreshed from a slot
    of either kind (left alone for best_slot = -1); ncommit = 0 with a best-row refresh runs one workgroup and writes no row."""
    N, nslot = 12, 16
    ldf = (n + 15) & ~15
    rng = np.random.default_rng(70 + n)
    TXf, TMf = np.zeros((nslot, ldf)), np.zeros((nslot, ldf))
    TXf[:, :n], TMf[:, :n] = rng.uniform(-1, 1, (nslot, n)), rng.uniform(1, 2, (nslot, n))
    dTX, dTM = DevBuf.from_array(TXf), DevBuf.from_array(TMf)
    slot, kind, row = np.array([3, 7, 11], np.int32), np.array([1, 2, 1], np.int32), np.array([5, 0, 9], np.int64)
    zb, guard = 4 * 37, 64
    colper, lay = shard_layout(n, world)
    for c0, nc, ld, _ in lay:
        Xs = np.zeros((N, ld))
        Xs[:, :nc] = rng.uniform(-9, -8, (N, nc))
        dXs = DevBuf.from_array(Xs)
        xb = np.full(ldf, 0.5)
        dxb = DevBuf.from_array(xb)
        for ncommit, bslot, bkind in ((3, 7, 2), (0, 3, 1), (2, -1, 1), (1, 11, 1)):
            blk = np.full(4 + zb + guard, 0xA5, np.uint8)
            dblk = DevBuf.from_array(blk)
            assert L.nla_k_crs_commit_sh(nc, ld, ldf, c0, dXs.ptr, dTX.ptr, dTM.ptr, ncommit, slot.ctypes.data, kind.ctypes.data, row.ctypes.data,
                                         dblk.ptr + 4, zb, n, bslot, bkind, dxb.ptr, None) == 0
            assert L.nla_stream_sync(None) == 0
            for c in range(ncommit):
                Xs[row[c], :nc] = (TXf if kind[c] == 1 else TMf)[slot[c], c0:c0 + nc]
            if bslot >= 0:
                xb[:n] = (TXf if bkind == 1 else TMf)[bslot, :n]
            assert np.array_equal(dXs.to_array(np.float64, N * ld).reshape(N, ld), Xs), (c0, ncommit)      # pad columns and other rows untouched
            assert np.array_equal(dxb.to_array(np.float64, ldf), xb), (c0, ncommit, bslot)
            got = dblk.to_array(np.uint8, 4 + zb + guard)
            assert not got[4:4 + zb].any() and np.all(got[:4] == 0xA5) and np.all(got[4 + zb:] == 0xA5)
        # refused before the launch: more commits than the kernel arguments hold, a byte count that is no multiple of 4
        big, bigrow = np.zeros(129, np.int32), np.zeros(129, np.int64)
        for ncommit, z in ((129, zb), (1, zb + 2), (-1, zb)):
            assert L.nla_k_crs_commit_sh(nc, ld, ldf, c0, dXs.ptr, dTX.ptr, dTM.ptr, ncommit, big.ctypes.data, big.ctypes.data,
                                         bigrow.ctypes.data, dblk.ptr + 4, z, n, 3, 1, dxb.ptr, None) != 0
        assert L.nla_stream_sync(None) == 0
        assert np.array_equal(dXs.to_array(np.float64, N * ld).reshape(N, ld), Xs) and np.array_equal(dxb.to_array(np.float64, ldf), xb)
    assert np.array_equal(dTX.to_array(np.float64, nslot * ldf).reshape(nslot, ldf), TXf)


def test_zz_report_largest_relative_differences():
    """(runs last in the module) the largest relative difference in f seen per launcher group, against the 1e-10 bound"""
    print("largest relative difference in f per group:", {k: "%.3g" % v for k, v in sorted(MAXREL.items())}, "bound", RTOL)
    assert all(v <= RTOL for v in MAXREL.values())
