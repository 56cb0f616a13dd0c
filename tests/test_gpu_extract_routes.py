"""GPU: cw_extract_piles_device held to the plain reference (tests/extract_ref.py) on the designed probes of tests/extract_probes.py, each alone in its call, on
the product library and on the -DCW_TEST_AIDS one: win_first_seq, seq_len and seq_word_off as numbers, the packed words word for word (padding bits
included), and the totals of the sizing call.  Then all geometry probes as the jobs of one call, capacities that are exact with guard words behind every
output array, capacities one short, the refusals, and the driver's composition of a job out of slices (csrc/cw_driver.cpp extract(): size every slice,
extract it at its place, move its offsets with cw_add_offsets_device) against the one-call extraction.  Integers throughout: every comparison is exact."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import consent_amd as ca
import extract_probes as pb
import extract_ref as xr
from consent_amd import engine as en
from extract_probes import BY_NAME, CATALOGUE, ref_of

pytestmark = pytest.mark.gpu

PRM = (9, 4, 8, 2, 20)
OK, E_INVALID, E_CAPACITY = 0, -1, -4
GUARD = 64
S32, S64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5
LIBRARIES = ("product", "aids")


@pytest.fixture(scope="module")
def engines():
    """One engine per library for the whole file: {"product": Engine, "aids": Engine}."""
    prev = en.use_library(en.AIDS_LIB)
    try:
        aids = ca.Engine(ca.Params(*PRM))
    finally:
        en._LIB = prev
    product = ca.Engine(ca.Params(*PRM))
    assert aids.lib is not product.lib
    for e in (aids, product):
        e.lib.cw_extract_impl.argtypes = [C.c_void_p, C.POINTER(en.ReadSet), C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.c_void_p]
        e.lib.cw_add_offsets_device.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
    yield {"product": product, "aids": aids}
    aids.close()
    product.close()


def up(a, dt):
    import torch

    a = np.ascontiguousarray(a)
    return torch.from_numpy((a if a.size else np.zeros(1, a.dtype)).view(dt)).to("cuda:0")


def sync():
    import torch

    torch.cuda.synchronize()


class Inputs:
    """A probe's read set, overlaps and jobs on the device."""

    def __init__(self, p):
        hb = ca.pack_piles([p.reads])
        self.keep = (up(hb.seq_len, np.int32), up(hb.seq_word_off, np.int64), up(np.concatenate([hb.bases, np.zeros(1, np.uint32)]), np.int32))
        self.reads = en.ReadSet(len(p.reads), *(t.data_ptr() for t in self.keep))
        self.ovl = up(np.array(p.ovl, np.uint32).reshape(-1, 6), np.int32)
        self.jobs_host = np.ascontiguousarray(np.array(p.jobs, np.uint32).reshape(-1, 5))
        self.jobs = up(self.jobs_host, np.int32)
        self.n_ovl, self.n_jobs, self.k = len(p.ovl), len(p.jobs), p.k


class Outputs:
    """The four output arrays, every element the sentinel, with GUARD elements behind each capacity."""

    def __init__(self, n_jobs, seq_cap, word_cap):
        self.n_jobs, self.seq_cap, self.word_cap = n_jobs, seq_cap, word_cap
        self.wfs = up(np.full(n_jobs + 1 + GUARD, S32, np.uint32), np.int32)
        self.len = up(np.full(seq_cap + GUARD, S32, np.uint32), np.int32)
        self.off = up(np.full(seq_cap + GUARD, S64, np.uint64), np.int64)
        self.bases = up(np.full(word_cap + GUARD, S32, np.uint32), np.int32)
        sync()  # the engine launches on its own stream: the fills above must have landed

    def ptrs(self, w0=0, seq_base=0, word_base=0):
        return self.wfs.data_ptr() + 4 * w0, self.len.data_ptr() + 4 * seq_base, self.off.data_ptr() + 8 * seq_base, self.bases.data_ptr() + 4 * word_base

    def host(self):
        sync()
        return (self.wfs.cpu().numpy().view(np.uint32), self.len.cpu().numpy().view(np.uint32), self.off.cpu().numpy().view(np.uint64), self.bases.cpu().numpy().view(np.uint32))

    def untouched(self):
        wfs, lens, offs, bases = self.host()
        return bool((wfs == S32).all() and (lens == S32).all() and (offs == S64).all() and (bases == S32).all())


def extract(eng, d, ptrs=(None, None, None, None), seq_cap=0, word_cap=0, w0=0, w1=None, k=None, through_impl=False):
    """One call over the jobs [w0, w1) of the inputs: (rc, n_seqs, n_words)."""
    w1 = d.n_jobs if w1 is None else w1
    ns, nw = C.c_uint32(0xDEAD), C.c_uint64(0xDEAD)
    head = (eng.handle, C.byref(d.reads), d.ovl.data_ptr(), d.n_ovl, d.jobs.data_ptr() + 20 * w0)
    tail = (w1 - w0, d.k if k is None else k, *ptrs, seq_cap, word_cap, C.byref(ns), C.byref(nw), None)
    if through_impl:  # the driver's entry: the same jobs in host memory as well
        rc = eng.lib.cw_extract_impl(*head, d.jobs_host.ctypes.data + 20 * w0, *tail)
    else:
        rc = eng.lib.cw_extract_piles_device(*head, *tail)
    return rc, ns.value, nw.value


@functools.lru_cache(maxsize=None)
def layout_of(name):
    """The reference's batch of a catalogue probe: computed once, shared, not changed."""
    return xr.layout([pile for pile, _ in ref_of(name)])


def check(out, exp):
    """The output arrays are the reference's batch, number for number and word for word, and nothing else was written."""
    wfs, lens, offs, words = exp
    g_wfs, g_len, g_off, g_bases = out.host()
    assert np.array_equal(g_wfs[: len(wfs)], wfs), np.flatnonzero(g_wfs[: len(wfs)] != wfs)[:5]
    assert np.array_equal(g_len[: len(lens)], lens), np.flatnonzero(g_len[: len(lens)] != lens)[:5]
    assert np.array_equal(g_off[: len(offs)], offs), np.flatnonzero(g_off[: len(offs)] != offs)[:5]
    assert np.array_equal(g_bases[: len(words)], words), np.flatnonzero(g_bases[: len(words)] != words)[:5]
    assert (g_wfs[len(wfs) :] == S32).all() and (g_len[len(lens) :] == S32).all() and (g_off[len(offs) :] == S64).all() and (g_bases[len(words) :] == S32).all()
    assert len(g_wfs) - len(wfs) == GUARD and len(g_len) - len(lens) >= GUARD and len(g_bases) - len(words) >= GUARD


def size_then_extract(eng, d, exp, **kw):
    """The sizing call (capacities 0, null outputs) and the call with exact capacities and guards."""
    wfs, lens, offs, words = exp
    assert extract(eng, d, **kw) == (E_CAPACITY, len(lens), len(words))
    out = Outputs(d.n_jobs, len(lens), len(words))
    assert extract(eng, d, out.ptrs(), len(lens), len(words), **kw) == (OK, len(lens), len(words))
    check(out, exp)
    return out


@pytest.mark.parametrize("name", list(BY_NAME))
def test_probe_alone(engines, name):
    p = BY_NAME[name]
    d = Inputs(p)
    for library in LIBRARIES:
        size_then_extract(engines[library], d, layout_of(name))


@pytest.mark.parametrize("library", LIBRARIES)
def test_more_shifts_longer_than_their_slice(engines, library):
    """Beside the catalogue's two throw probes (their number is fixed): the '+' twin of the second, and on both strands a slice that begins exactly on the
    read's end under a shift -- `substr` at pos == size gives an empty slice, which the shift then exceeds.  The reference would throw; restatement, oracle
    and kernel give the template alone."""
    import oracle_lib

    probes = pb.geo("shift beyond the cut slice", (40, 150, 145, 250), {"inside", "substr_clamp", "throw_shift"}, strands=(0,), throws=True)
    probes += pb.geo("shift beyond an empty slice", (40, 150, 150, 260), {"inside", "substr_clamp", "throw_shift"}, throws=True)
    for p in probes:
        (pile, notes), = p.reference()
        assert len(pile) == 1 and [set(n) for n in notes] == p.notes[0]
        assert pile == oracle_lib.window_pile(oracle_lib.oracle().cwo_window_pile, *p.job_inputs(0), p.k)
        size_then_extract(engines[library], Inputs(p), xr.layout([pile]))


def geometry_by_k():
    groups = {}
    for p in CATALOGUE:
        if p.kind == "geometry":
            groups.setdefault(p.k, []).append(p)
    assert sorted(groups) == [1, 9, 16] and len(groups[9]) > 60
    return groups


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("library", LIBRARIES)
def test_the_geometry_probes_as_the_jobs_of_one_call(engines, library, order):
    """One shared read set, every probe's window a job (a call has one k: the probes of k = 1 and k = 16 make calls of their own), as written and shuffled."""
    for k, probes in geometry_by_k().items():
        probes = list(probes)
        if order:
            random.Random(order).shuffle(probes)
        m = pb.merged("geometry", probes)
        exp = xr.layout([pile for q in probes for pile, _ in ref_of(q.name)])
        assert len(m.jobs) == len(exp[0]) - 1
        size_then_extract(engines[library], Inputs(m), exp)


@pytest.mark.parametrize("name", ["129 overlaps", "kept and dropped alternating", "5 jobs", "inside: a window of 1040 bases (-)", "1025 jobs, the last pile empty"])
@pytest.mark.parametrize("library", LIBRARIES)
def test_a_capacity_one_short_writes_nothing(engines, library, name):
    """seq_cap one short, and word_cap one short: CW_E_CAPACITY, the totals reported, and no element of the four arrays written -- win_first_seq included."""
    d, (wfs, lens, offs, words) = Inputs(BY_NAME[name]), layout_of(name)
    for seq_cap, word_cap in ((len(lens) - 1, len(words)), (len(lens), len(words) - 1)):
        out = Outputs(d.n_jobs, len(lens), len(words))
        assert extract(engines[library], d, out.ptrs(), seq_cap, word_cap) == (E_CAPACITY, len(lens), len(words))
        assert out.untouched()


@pytest.mark.parametrize("library", LIBRARIES)
def test_refusals(engines, library):
    eng, p = engines[library], BY_NAME["three jobs of one template share one overlap range"]
    d = Inputs(p)
    out = Outputs(d.n_jobs, 16, 64)
    assert extract(eng, d, out.ptrs(), 16, 64, w1=0) == (OK, 0, 0) and out.untouched()  # no job: nothing to do

    def refused(jobs=None, **kw):
        bad = Inputs(pb.Probe("bad", p.reads, p.ovl, jobs or p.jobs))
        return extract(eng, bad, out.ptrs(), 16, 64, **kw)[0] == E_INVALID and out.untouched()

    assert refused([[0, 0, 49, 0, 3], [0, 45, 94, 1, 3]])      # ovl_first + ovl_count > n_overlaps
    assert refused([[0, 0, 49, 0, 3], [0, 45, 94, 0xFFFFFFFF, 2]])  # ... the sum taken in 64 bits
    assert refused([[0, 0, 49, 0, 3], [4, 45, 94, 0, 3]])      # tpl_read >= n_reads
    assert refused([[0, 0, 49, 0, 3], [0, 45, 44, 0, 3]])      # q_end < q_beg
    assert refused(k=0)
    (wfs, lens, offs, words) = layout_of(p.name)  # ... and the engine is none the worse for them
    assert extract(eng, d, out.ptrs(), 16, 64) == (OK, len(lens), len(words)) and len(lens) <= 16 and len(words) <= 64
    g = out.host()
    assert np.array_equal(g[0][: len(wfs)], wfs) and np.array_equal(g[1][: len(lens)], lens) and np.array_equal(g[3][: len(words)], words)


# ---- slices and offsets: csrc/cw_driver.cpp extract() -----------------------------------------------------------------------------------------------------

def add_offsets(eng, a32, n32, add32, a64, n64, add64):
    return eng.lib.cw_add_offsets_device(a32, n32, add32, a64, n64, add64, None)


def compose(eng, d, bounds, through_impl=False):
    """The jobs cut at `bounds` into slices, as the driver does it: size every slice, extract each at its seq_base / word_base with offsets that start at
    zero, move them to the slice's place."""
    slices, tot_seqs, tot_words = [], 0, 0
    for w0, w1 in zip(bounds, bounds[1:]):
        rc, ns, nw = extract(eng, d, w0=w0, w1=w1, through_impl=through_impl)
        assert rc in (OK, E_CAPACITY)
        slices.append((w0, w1, ns, nw, tot_seqs, tot_words))
        tot_seqs, tot_words = tot_seqs + ns, tot_words + nw
    out = Outputs(d.n_jobs, tot_seqs, tot_words)
    for w0, w1, ns, nw, seq_base, word_base in slices:
        wfs, lens, offs, bases = out.ptrs(w0, seq_base, word_base)
        assert extract(eng, d, (wfs, lens, offs, bases), ns, nw, w0=w0, w1=w1, through_impl=through_impl) == (OK, ns, nw)
        sync()  # (the driver has both on one stream; here the extraction runs on the engine's and the move on the null stream)
        assert add_offsets(eng, wfs, w1 - w0 + 1, seq_base, offs, ns, word_base) == OK
        sync()
    return out, slices


def pile_jobs():
    probes = [p for p in CATALOGUE if p.kind == "pile"]
    assert any(p.name == "129 overlaps" for p in probes)
    return pb.merged("piles", probes), xr.layout([pile for q in probes for pile, _ in ref_of(q.name)])


@pytest.mark.parametrize("library", LIBRARIES)
def test_slices_compose_to_the_one_call_extraction(engines, library):
    eng = engines[library]
    big = "2049 jobs, the piles of jobs 0, 1024 and 2048 empty"
    m, m_exp = pile_jobs()
    n = len(m.jobs)
    assert n >= 8
    cases = [(Inputs(BY_NAME[big]), layout_of(big), [[0, 2049], [0, 1024, 2049], [0, 1, 300, 1024, 1025, 1500, 2048, 2049]]),  # (0,1), (1024,1025), (2048,2049): one job, an empty pile
             (Inputs(m), m_exp, [[0, n], [0, 6, n], [0, 1, 2, 5, 6, 7, n - 1, n]])]
    for d, exp, cuts in cases:
        one_call = size_then_extract(eng, d, exp).host()
        for bounds in cuts:
            out, slices = compose(eng, d, bounds)
            assert len(slices) in (1, 2, 7)
            check(out, exp)
            assert all(np.array_equal(a, b) for a, b in zip(out.host(), one_call))
    d, exp, cuts = cases[0]
    assert any(w1 - w0 == 1 and ns == 0 for w0, w1, ns, _, _, _ in compose(eng, d, cuts[2])[1])  # a slice of one job that is all empty piles
    out, _ = compose(eng, d, cuts[2], through_impl=True)  # the driver's own entry, the jobs handed over in host memory too
    check(out, exp)


@pytest.mark.parametrize("library", LIBRARIES)
def test_a_slice_of_nothing_but_empty_piles_between_two_others(engines, library):
    """Three templates, the second one shorter than its four windows."""
    reads = [pb.rand_seq("slice/a", 120), pb.rand_seq("slice/b", 30), pb.rand_seq("slice/c", 120), pb.rand_seq("slice/target", 150)]
    ovl = [[0, 119, 3, 10, 129, 0], [0, 29, 3, 0, 29, 1], [0, 119, 3, 20, 139, 1]]
    jobs = [[0, 10, 59, 0, 1], [0, 60, 109, 0, 1]] + [[1, 5 * i, 5 * i + 49, 1, 1] for i in range(4)] + [[2, 10, 59, 2, 1], [2, 60, 109, 2, 1]]
    p = pb.Probe("empty slice", reads, ovl, jobs)
    ref = p.reference()
    assert [len(pile) for pile, _ in ref] == [2, 2, 0, 0, 0, 0, 2, 2]
    exp = xr.layout([pile for pile, _ in ref])
    out, slices = compose(engines[library], Inputs(p), [0, 2, 6, 8])
    assert slices[1][2:4] == (0, 0)
    check(out, exp)


@pytest.mark.parametrize("library", LIBRARIES)
def test_add_offsets(engines, library):
    eng = engines[library]
    rng = np.random.default_rng(3)
    g = 8  # guard elements on both sides
    for n32, n64 in ((255, 255), (256, 256), (257, 257), (255, 257), (257, 255), (1, 600), (600, 1), (0, 257), (257, 0)):
        for add32, add64 in ((7, (1 << 32) + 5), (0, 1 << 40), (3, 0), (0, 0)):
            a32, a64 = rng.integers(0, 1 << 31, n32 + 2 * g, dtype=np.uint32), rng.integers(0, 1 << 62, n64 + 2 * g, dtype=np.uint64)
            t32, t64 = up(a32, np.int32), up(a64, np.int64)
            sync()
            assert add_offsets(eng, t32.data_ptr() + 4 * g, n32, add32, t64.data_ptr() + 8 * g, n64, add64) == OK
            sync()
            e32, e64 = a32.copy(), a64.copy()
            e32[g : g + n32] += np.uint32(add32)
            e64[g : g + n64] += np.uint64(add64)
            assert np.array_equal(t32.cpu().numpy().view(np.uint32), e32) and np.array_equal(t64.cpu().numpy().view(np.uint64), e64), (n32, n64, add32, add64)
    assert add_offsets(eng, None, 0, 5, None, 0, 5) == OK  # nothing to move
    t = up(np.zeros(4, np.uint64), np.int64)
    assert add_offsets(eng, None, 4, 5, t.data_ptr(), 4, 5) == E_INVALID and add_offsets(eng, t.data_ptr(), 4, 5, None, 4, 5) == E_INVALID
    assert add_offsets(eng, None, 0, 5, t.data_ptr(), 4, 5) == OK  # (a null array of no elements is none)
    sync()
    assert t.cpu().numpy().tolist() == [5, 5, 5, 5]
