"""-m gpu: the GATED pair of kernels every constrained ISRES generation on one device ranks through (isres_driver.c, dev_rank_bits_gated /
dev_rank): nla_k_mt_rankbits_gated (hip/mt_kernels.hip, mt_rankbits_kernel with gate / ticket) produces the u < 0.45 bits on the
generator's stream and counts, per block of 64 sweeps, the wavefronts that have delivered all they owe to it; nla_k_isres_stochrank_gated
(hip/isres_stochrank.h) starts beside it and its unit u waits until gate[u] reaches a target it recomputes inline.  The other ISRES tests
reach the ungated forms only, and end to end a broken gated path hides behind the driver's fallback (a unit that gives up -> the ranking is
done again without gates, the result is right).

Everything here is an integer or a bit: every assertion is exact.  Expectations: the serial generator of oracle/'s port turned into bits
with numpy, a brute-force count of the stream segments that intersect a block's words, the reference's double loop in Python
(test_gpu_isres._serial_stochrank) and the library's ungated kernels, which tests/test_gpu_kernels.py and tests/test_gpu_isres.py pin.

gate: units + 3 ints of ordinary device memory as the driver's (units = ceil(pop / 64)): gate[0 .. units) the counters, gate[units + 1] the
generator's ticket, gate[units + 2] the word a unit of the pipeline sets when it gives up waiting."""
import ctypes as C
import functools

import numpy as np
import pytest

import nlopt_amd
from nlopt_amd import DevBuf
from test_gpu_isres import _serial_stochrank
from test_gpu_kernels import words_from_seed

pytestmark = pytest.mark.gpu
SEG = 624 * 1024                  # words per segment of the device stream (NLA_MT_SEG_WORDS)

# name -> (pop, stream index of the ranking's first word, seed, words drawn from the host generator before the stream is created).
# The stream's origin is the number of words drawn from the current regeneration (predraw here, < 624), the rest is rel_rank0.
CASES = {
    "pop2": (2, 0, 9, 0),                          # one step per sweep, one unit, target 1
    "pop65": (65, 2 * SEG - 8255, 5489, 1),        # rows of exactly one word; unit 1 is ONE sweep whose 128 words straddle segments 1 | 2: targets
                                                   # {1, 2}; odd: a step has its first word in segment 1 and its second in segment 2
    "pop300": (300, SEG - 1000, 42, 0),            # block 0 straddles segments 0 | 1: targets {2, 1, 1, 1, 1}; rows end inside a word
    "pop777": (777, 3 * SEG - 5, 7, 3),            # odd; 13 units over 3 segments, the last unit has 9 sweeps
    "pop1500": (1500, 623, 123456789, 623),        # 24 units, 8 segments: several blocks inside one segment
    "pop5000": (5000, SEG - 500, 11, 0),           # a block (639 872 words) is longer than a segment: block 0 spans 3, later ones 2; 80 segments, 79 units
    # not in the issue's table: block 0 ENDS exactly on a segment boundary (its last word is the last word of segment 0, the gate moves at the
    # segment's last regeneration), unit 1's single sweep is the first 128 words of segment 1
    "pop65_block0_fills_segment0": (65, SEG - 128 * 64, 77, 0),
}
WHAT_THE_TABLE_SAYS = {"pop2": [1], "pop65": [1, 2], "pop300": [2, 1, 1, 1, 1], "pop65_block0_fills_segment0": [1, 1]}


def geometry(name):
    pop, g_rank0, seed, predraw = CASES[name]
    popm1 = pop - 1
    return dict(name=name, pop=pop, popm1=popm1, g_rank0=g_rank0, seed=seed, predraw=predraw, rel=g_rank0 - predraw,
                roww=(popm1 + 63) // 64, units=(pop + 63) // 64, count=2 * popm1 * pop)


def segments_touched(b0, b1):
    """how many segments [s SEG, (s + 1) SEG) have a word in [b0, b1): counted one by one"""
    return sum(1 for s in range(b1 // SEG + 2) if max(s * SEG, b0) < min((s + 1) * SEG, b1))


def brute_target(g_rank0, popm1, nrows, c):
    b0 = g_rank0 + 128 * popm1 * c
    b1 = g_rank0 + 2 * popm1 * min(64 * (c + 1), nrows)
    return segments_touched(b0, b1)


def brute_targets(g):
    return [brute_target(g["g_rank0"], g["popm1"], g["pop"], c) for c in range(g["units"])]


@pytest.fixture(scope="module")
def L():
    L = nlopt_amd.lib()
    assert nlopt_amd.device_count() > 0, "no HIP device: the product has no CPU fallback"
    vp = C.c_void_p
    L.nla_rankbits_gate_target.argtypes = [C.c_uint64, C.c_int64, C.c_int64, C.c_int64]
    L.nla_mtstream_origin.argtypes = [vp]
    L.nla_mtstream_origin.restype = C.c_uint64
    L.nla_mtstream_rankbits_gated.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int64, C.c_int64, vp, vp, vp, C.c_int]
    L.nla_stream_wait_event.argtypes = [vp, vp]
    return L


def open_stream(L, g, stream):
    """the host generator seeded and drawn from as the case says, continued on the device: the ranking's first word is stream word g_rank0"""
    L.nlopt_srand(g["seed"])
    for _ in range(g["predraw"]):
        L.nla_genrand_int32()
    s = L.nla_mtstream_create(stream)
    assert s
    assert L.nla_mtstream_origin(s) + g["rel"] == g["g_rank0"]
    return s


@functools.lru_cache(maxsize=None)
def expected_bits(name):
    """pop x rowwords words from the serial generator: bit j of row i = nlopt_urand(0,1) < 0.45 of step i (pop - 1) + j (isres.c:210), the
    expression of tests/test_gpu_kernels.py; pad bits beyond pop - 1 in a row's last word are zero.  Computed once, read-only."""
    g = geometry(name)
    pop, popm1, roww = g["pop"], g["popm1"], g["roww"]
    ref = words_from_seed(g["seed"], g["rel"] + g["count"], skip=g["predraw"])[g["rel"]:]
    out = np.zeros((pop, roww), np.uint64)
    for r0 in range(0, pop, 512):                  # (in slabs of rows: the intermediates of 5e7 words at once are gigabytes)
        r1 = min(r0 + 512, pop)
        w = ref[2 * popm1 * r0:2 * popm1 * r1].astype(np.uint64)
        u = ((w[0::2] >> np.uint64(5)) * 67108864.0 + (w[1::2] >> np.uint64(6)).astype(np.float64)) * (1.0 / 9007199254740992.0)
        want = np.zeros((r1 - r0, roww * 64), bool)
        want[:, :popm1] = (u < 0.45).reshape(r1 - r0, popm1)
        out[r0:r1] = np.packbits(want.reshape(r1 - r0, roww, 64), axis=2, bitorder="little").view(np.uint64).reshape(r1 - r0, roww)
    out.setflags(write=False)
    return out


def assert_bits(dbits, g):
    want = expected_bits(g["name"])
    got = dbits.to_array(np.uint64, g["pop"] * g["roww"]).reshape(g["pop"], g["roww"])
    bad = np.argwhere(got != want)
    assert len(bad) == 0, ("%d words differ, the first in row %d word %d" % (len(bad), bad[0][0], bad[0][1]),
                           hex(int(got[tuple(bad[0])])), hex(int(want[tuple(bad[0])])))


def assert_gate(dgate, g, gave_up=0):
    units = g["units"]
    gate = dgate.to_array(np.int32, units + 3)
    nseg = segments_touched(g["g_rank0"], g["g_rank0"] + g["count"])
    assert gate[:units].tolist() == brute_targets(g)         # exactly: one short and a unit waits for ever, one over and it reads an unfinished row
    assert gate[units] == 0
    assert gate[units + 1] == nseg                           # the ticket: one per segment launched
    assert gate[units + 2] == gave_up


def gate_target_cases():
    """the table, and for every population of it streams laid so that a block starts exactly on a segment boundary (the block in front
    then ends on it) and so that the last block ends on one"""
    out = [(k, CASES[k][0], CASES[k][1]) for k in CASES]
    for pop in sorted({CASES[k][0] for k in CASES}):
        popm1, units = pop - 1, (pop + 63) // 64
        for c in sorted({0, 1, units // 2, units - 1}):
            k = (128 * popm1 * c) // SEG + 1
            out.append(("pop%d_block%d_starts_on_boundary" % (pop, c), pop, k * SEG - 128 * popm1 * c))
        k = (2 * popm1 * pop) // SEG + 2
        out.append(("pop%d_ends_on_boundary" % pop, pop, k * SEG - 2 * popm1 * pop))
    return out


@pytest.mark.parametrize("name,pop,g_rank0", gate_target_cases(), ids=[c[0] for c in gate_target_cases()])
def test_gate_target_against_a_brute_force_count(L, name, pop, g_rank0):
    """nla_rankbits_gate_target (a host function of the device library: no launch) = the number of segments that hold a word of sweeps
    64 c .. min(64 c + 64, pop) - 1, counted segment by segment; 0 for c = units."""
    popm1, units = pop - 1, (pop + 63) // 64
    got = [L.nla_rankbits_gate_target(g_rank0, popm1, pop, c) for c in range(units + 1)]
    assert got == [brute_target(g_rank0, popm1, pop, c) for c in range(units)] + [0]
    assert all(t >= 1 for t in got[:units])
    if name in WHAT_THE_TABLE_SAYS:
        assert got[:units] == WHAT_THE_TABLE_SAYS[name]
    if name == "pop5000":
        assert got[0] == 3 and set(got[1:units - 1]) == {2} and units == 79       # (the last unit: 8 sweeps)
    if "starts_on_boundary" in name:
        c = int(name.split("_block")[1].split("_")[0])
        assert (g_rank0 + 128 * popm1 * c) % SEG == 0
    if name.endswith("_ends_on_boundary"):
        assert (g_rank0 + 2 * popm1 * pop) % SEG == 0


@pytest.mark.parametrize("wpc", [0, 8, 1], ids=["wpc0", "wpc8", "wpc1"])
@pytest.mark.parametrize("name", list(CASES))
def test_gated_generator_alone(L, name, wpc):
    """nla_mtstream_rankbits_gated on the default stream, nothing beside it; waves_per_cu as the plain launch (0), as the driver (8) and one
    wavefront per compute unit (1).  Bits word for word against the serial generator and against the ungated launch, every gate exactly at
    its target, the ticket at the number of segments, nobody gave up.  Twice on the same buffers."""
    g = geometry(name)
    pop, popm1, roww, units = g["pop"], g["popm1"], g["roww"], g["units"]
    s = open_stream(L, g, None)
    dbits, dgate = DevBuf(8 * pop * roww), DevBuf(4 * (units + 3))
    try:
        for rep in range(2):
            assert L.nla_memset(dbits.ptr, 0, 8 * pop * roww, None) == 0 and L.nla_memset(dgate.ptr, 0, 4 * (units + 3), None) == 0
            assert L.nla_mtstream_rankbits_gated(s, g["rel"], g["rel"], g["count"], popm1, roww, dbits.ptr, dgate.ptr,
                                                 dgate.ptr + 4 * (units + 1), wpc) == 0
            assert L.nla_stream_sync(None) == 0
            assert_bits(dbits, g)
            assert_gate(dgate, g)
        d2 = DevBuf.from_array(np.zeros(pop * roww, np.uint64))
        assert L.nla_mtstream_rankbits(s, g["rel"], g["rel"], g["count"], popm1, roww, d2.ptr) == 0
        assert L.nla_stream_sync(None) == 0
        assert np.array_equal(d2.to_array(np.uint64, pop * roww), dbits.to_array(np.uint64, pop * roww))
        d2.free()
    finally:
        L.nla_mtstream_destroy(s)
        dbits.free()
        dgate.free()


class Pipeline:
    """the ranking pipeline's buffers for one population: values with many ties (as tests/test_gpu_isres.py), the packed elements"""

    def __init__(self, L, pop, seed):
        rng = np.random.default_rng(seed)
        self.L, self.pop, self.units = L, pop, (pop + 63) // 64
        self.f = rng.integers(0, pop // 2 + 2, pop).astype(np.float64)
        self.pen = np.where(rng.random(pop) < 0.4, 0.0, rng.integers(1, 6, pop).astype(np.float64))
        self.dF, self.dP = DevBuf.from_array(self.f), DevBuf.from_array(self.pen)
        self.dstreams, self.dsorted = DevBuf(8 * (self.units + 1) * pop), DevBuf(4 * pop)
        self.dsw, self.dirank = DevBuf(pop), DevBuf(4 * pop)
        self.prog = np.zeros(self.units + 1, np.int32)
        self.prog[0] = pop
        self.dprog, self.dticket = DevBuf(4 * (self.units + 1)), DevBuf(4)

    def count(self, stream):
        assert self.L.nla_k_isres_rank_count(self.pop, self.dF.ptr, self.dP.ptr, self.dstreams.ptr, self.dsorted.ptr, stream) == 0

    def reset(self, stream):
        """progress and ticket as the driver sets them in front of every launch; the outputs to values no run leaves behind"""
        L = self.L
        assert L.nla_memcpy_h2d(self.dprog.ptr, self.prog.ctypes.data, self.prog.nbytes, stream) == 0
        assert L.nla_memset(self.dticket.ptr, 0, 4, stream) == 0
        assert L.nla_memset(self.dsw.ptr, 0xEE, self.pop, stream) == 0 and L.nla_memset(self.dirank.ptr, 0xFF, 4 * self.pop, stream) == 0

    def launch(self, nsweeps, dbits, gate_ptr, g_rank0, stream):
        assert self.L.nla_k_isres_stochrank_gated(self.pop, nsweeps, self.dstreams.ptr, self.dprog.ptr, dbits.ptr, self.dticket.ptr, self.dsw.ptr,
                                                  self.dirank.ptr, gate_ptr, g_rank0, self.pop if gate_ptr else 0, stream) == 0

    def results(self, nsweeps):
        return self.dsw.to_array(np.uint8, self.pop)[:nsweeps].copy(), self.dirank.to_array(np.int32, self.pop)

    def ungated(self, nsweeps, dbits):
        L = self.L
        self.reset(None)
        assert L.nla_k_isres_stochrank(self.pop, nsweeps, self.dstreams.ptr, self.dprog.ptr, dbits.ptr, self.dticket.ptr, self.dsw.ptr,
                                       self.dirank.ptr, None) == 0
        assert L.nla_stream_sync(None) == 0
        return self.results(nsweeps)

    def free(self):
        for b in (self.dF, self.dP, self.dstreams, self.dsorted, self.dsw, self.dirank, self.dprog, self.dticket):
            b.free()


@pytest.mark.parametrize("name", ["pop2", "pop65", "pop300", "pop777", "pop1500"])
def test_gated_pipeline_with_the_gates_already_at_their_targets(L, name):
    """nla_k_isres_stochrank_gated on complete bits with gate[] filled by the HOST with the brute-force targets: the same swapped[] and irank
    as nla_k_isres_stochrank on the same inputs, and nobody gave up — were the kernel's inline target larger than the count for one unit,
    that unit would wait its 4 s out and set the word.  pop <= 300: also the reference's double loop in Python on the same bits (the ranking
    after exactly the sweeps the reference takes, as tests/test_gpu_isres.py does it); above that the loop is too slow and the ungated kernel,
    which that test pins, is the expectation."""
    g = geometry(name)
    pop, popm1, roww, units = g["pop"], g["popm1"], g["roww"], g["units"]
    s = open_stream(L, g, None)
    dbits = DevBuf.from_array(np.zeros(pop * roww, np.uint64))
    dgate = DevBuf.from_array(np.zeros(units + 3, np.int32))
    p = Pipeline(L, pop, 100 + pop)
    try:
        assert L.nla_mtstream_rankbits_gated(s, g["rel"], g["rel"], g["count"], popm1, roww, dbits.ptr, dgate.ptr, dgate.ptr + 4 * (units + 1), 8) == 0
        assert L.nla_stream_sync(None) == 0
        assert_bits(dbits, g)
        p.count(None)
        sw0, ir0 = p.ungated(pop, dbits)
        assert sorted(ir0.tolist()) == list(range(pop))
        gate = np.array(brute_targets(g) + [0, 0, 0], np.int32)

        def gated(nsweeps):
            assert L.nla_memcpy_h2d(dgate.ptr, gate.ctypes.data, gate.nbytes, None) == 0
            p.reset(None)
            p.launch(nsweeps, dbits, dgate.ptr, g["g_rank0"], None)
            assert L.nla_stream_sync(None) == 0
            after = dgate.to_array(np.int32, units + 3)
            assert after[units + 2] == 0, "a unit gave up waiting although every gate stood at its target"
            assert np.array_equal(after, gate)               # (the pipeline only reads the counters)
            return p.results(nsweeps)

        sw1, ir1 = gated(pop)
        assert np.array_equal(sw1, sw0) and np.array_equal(ir1, ir0)
        if pop <= 300:
            low = np.unpackbits(expected_bits(name).view(np.uint8).reshape(pop, roww * 8), axis=1, bitorder="little")
            ref, sweeps = _serial_stochrank(p.f, p.pen, lambda i, j: bool(low[i, j]), pop, pop)
            first_quiet = next((i for i in range(pop) if not sw1[i]), pop)
            assert first_quiet + 1 == sweeps or (first_quiet == pop and sweeps == pop)
            sw2, ir2 = gated(sweeps)                         # (fewer units; the targets still count all pop sweeps the generator was asked for)
            assert ir2.tolist() == ref and np.array_equal(sw2, sw0[:sweeps])
            assert p.ungated(sweeps, dbits)[1].tolist() == ref
    finally:
        L.nla_mtstream_destroy(s)
        p.free()
        dbits.free()
        dgate.free()


@pytest.mark.parametrize("name", ["pop300", "pop1500", "pop5000"])
def test_generator_and_pipeline_side_by_side_in_the_drivers_order(L, name):
    """isres_driver.c, dev_rank_bits_gated and dev_rank.  On the generator's stream: bits and gate cleared, an event, the gated generator with
    the driver's waves_per_cu = 8.  On the main stream: rank counting, progress / ticket reset, wait for the event (the counters are zero
    before a unit looks at them), the gated pipeline on the real gate.  The generator is enqueued FIRST.  One launch: nobody gave up, the gates
    at their targets, the bits those of the serial generator, swapped[] and irank those of the ungated pipeline on the finished bits."""
    g = geometry(name)
    pop, popm1, roww, units = g["pop"], g["popm1"], g["roww"], g["units"]
    rs, st = L.nla_stream_create(), L.nla_stream_create()
    assert rs and st
    ev = L.nla_event_create()
    assert ev
    s = open_stream(L, g, rs)
    dbits, dgate = DevBuf(8 * pop * roww), DevBuf(4 * (units + 3))
    p = Pipeline(L, pop, 200 + pop)
    try:
        assert L.nla_memset(dbits.ptr, 0, 8 * pop * roww, rs) == 0 and L.nla_memset(dgate.ptr, 0, 4 * (units + 3), rs) == 0
        assert L.nla_event_record(ev, rs) == 0
        assert L.nla_mtstream_rankbits_gated(s, g["rel"], g["rel"], g["count"], popm1, roww, dbits.ptr, dgate.ptr, dgate.ptr + 4 * (units + 1), 8) == 0
        p.count(st)
        p.reset(st)
        assert L.nla_stream_wait_event(st, ev) == 0
        p.launch(pop, dbits, dgate.ptr, g["g_rank0"], st)
        assert L.nla_stream_sync(st) == 0 and L.nla_stream_sync(rs) == 0
        assert_gate(dgate, g)                                # (with the gave-up word at 0)
        assert_bits(dbits, g)
        sw1, ir1 = p.results(pop)
        sw0, ir0 = p.ungated(pop, dbits)
        assert sorted(ir0.tolist()) == list(range(pop))
        assert np.array_equal(sw1, sw0) and np.array_equal(ir1, ir0)
    finally:
        L.nla_mtstream_destroy(s)
        L.nla_event_destroy(ev)
        L.nla_stream_destroy(rs)
        L.nla_stream_destroy(st)
        p.free()
        dbits.free()
        dgate.free()
