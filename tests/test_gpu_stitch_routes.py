"""GPU: cw_stitch_kernel held to the plain reference (tests/stitch_ref.py) on the designed probes of tests/stitch_probes.py, each alone in its launch, on the
product library and on the -DCW_TEST_AIDS one: string and status; on the test-aid library also all eight trace words of every window an alignment was tried
for, the numbers of the overlap reconciliation, and the witnessed route of every window and of the read against the reference's and the hand-written one
(csrc/cw_stitch.h CwStRoute / CwStBand / CwStRead).  Then launches of many reads -- every wave takes several into the LDS another one used --, out slots with
guard bytes behind them, and the union of the witnessed bits.  Integers and bytes: every comparison is exact.

A launch has one geometry (k, window size, overlap, trimming): the launches of many reads take the probes of the default geometry; a probe of another geometry
is launched alone."""
import contextlib
import os
import random

import numpy as np
import pytest

import consent_amd as ca
import stitch_probes as pb
import stitch_ref as sr
from consent_amd import engine as en
from test_stitch_ref_cpu import BY_NAME, CATALOGUE, ref_of

pytestmark = pytest.mark.gpu

PRM = (pb.K, 4, 8, 2, 150)
NOT_REACHED = 0xFFFFFFFF


@pytest.fixture(scope="module")
def engines():
    """One engine per library for the whole file (every probe has k = 9): {"product": Engine, "aids": Engine}."""
    prev = en.use_library(en.AIDS_LIB)
    try:
        aids = ca.Engine(ca.Params(*PRM))
    finally:
        en._LIB = prev
    product = ca.Engine(ca.Params(*PRM))
    assert aids.lib is not product.lib
    yield {"product": product, "aids": aids}
    aids.close()
    product.close()


@contextlib.contextmanager
def traced():
    old = os.environ.get("CW_STITCH_TRACE")
    os.environ["CW_STITCH_TRACE"] = "1"
    try:
        yield
    finally:
        if old is None:
            del os.environ["CW_STITCH_TRACE"]
        else:
            os.environ["CW_STITCH_TRACE"] = old


def launch(eng, probes, caps=None):
    """The probes (of one geometry) as one launch: [(string, status)]."""
    p0 = probes[0]
    assert all((p.k, p.ws, p.wo, p.do_trim) == (p0.k, p0.ws, p0.wo, p0.do_trim) for p in probes)
    reads, jobs, pos, batch, res = pb.results_of(probes)
    return eng.stitch(reads, jobs, pos, batch, res, p0.ws, p0.wo, p0.do_trim, capacity=caps)


def names_of(word, table):
    return set() if word == NOT_REACHED else {n for n, b in table.items() if word & b}


def check_witness(eng, probes, seen=None):
    """Trace words, reconciliation numbers and routes of the last launch (the test-aid library, traced) against the reference's."""
    trace = eng.stitch_trace()
    win, rd = eng.stitch_route()
    w0 = 0
    for ri, p in enumerate(probes):
        r = ref_of(p.name)
        assert names_of(int(rd[ri]), en.STITCH_READ) == r.route, (p.name, names_of(int(rd[ri]), en.STITCH_READ), r.route)
        if seen is not None:
            seen["read"] |= names_of(int(rd[ri]), en.STITCH_READ)
        for w, rw in enumerate(r.windows):
            t, rec = trace[w0 + w], win[w0 + w]
            if rw.trace is None:
                assert (t == NOT_REACHED).all(), (p.name, w, t)
            else:
                assert tuple(int(x) for x in t.view(np.int32)) == rw.trace, (p.name, w, t.view(np.int32), rw.trace)
            got = names_of(int(rec[0]), en.STITCH_ROUTE) | names_of(int(rec[1]), en.STITCH_BAND)
            assert got == rw.route, (p.name, w, sorted(got ^ rw.route))
            if w in p.expect:
                assert got == p.expect[w], (p.name, w, sorted(got ^ p.expect[w]))
            # (a word left at 0xFFFFFFFF was not reached -- but the gap's move may BE -1: it is there exactly when the window was replaced)
            facts = {f: int(v) for f, v in zip(en.STITCH_FACTS, rec[2:].view(np.int32)) if int(v) != -1 or (f == "gap_move" and got & {"replaced_longer", "replaced_shorter", "replaced_same"})}
            assert facts == {f: v for f, v in rw.facts.items() if f != "bands"}, (p.name, w, facts, rw.facts)
            if seen is not None:
                seen["window"] |= got
        w0 += len(r.windows)


@pytest.mark.parametrize("name", list(BY_NAME))
def test_probe_alone(engines, name):
    p, r = BY_NAME[name], ref_of(name)
    caps = None if p.cap is None else [p.cap]
    got = launch(engines["product"], [p], caps)
    assert got == [(r.string, r.status)], (got[0][1], r.status, len(got[0][0]), len(r.string))
    with traced():  # the product library reads no test aid: nothing is recorded
        assert launch(engines["product"], [p], caps) == [(r.string, r.status)]
    assert engines["product"].stitch_route() is None
    with traced():
        got = launch(engines["aids"], [p], caps)
    assert got == [(r.string, r.status)], (got[0][1], r.status, len(got[0][0]), len(r.string))
    check_witness(engines["aids"], [p])
    launch(engines["aids"], [p], caps)  # without the switch the test-aid library records nothing either
    assert engines["aids"].stitch_route() is None


def default_class(do_trim=True):
    return [p for p in CATALOGUE if (p.k, p.ws, p.wo, p.do_trim) == (pb.K, 100, 10, do_trim) and p.cap is None]


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("library", ["product", "aids"])
def test_the_catalogue_repeated_and_shuffled_in_one_launch(engines, library, order):
    """More reads than the launch has waves (256 work-groups of four): every wave takes several reads into the LDS that held another's, and each read
    comes out with the bytes it gives alone."""
    probes = default_class()
    probes = probes * (1100 // len(probes) + 1)
    random.Random(order).shuffle(probes)
    assert len(probes) > 1024
    got = launch(engines[library], probes)
    for p, g in zip(probes, got):
        r = ref_of(p.name)
        assert g == (r.string, r.status), p.name


def test_the_untrimmed_probes_in_one_launch_with_their_witness(engines):
    probes = default_class(do_trim=False)
    with traced():
        got = launch(engines["aids"], probes)
    assert got == [(ref_of(p.name).string, ref_of(p.name).status) for p in probes]
    check_witness(engines["aids"], probes)


@pytest.mark.parametrize("library", ["product", "aids"])
def test_long_reads_of_the_order_kernels_last_class_with_short_ones(engines, library):
    """Reads of 1022, 1023, 1024 and 1500 windows (the order kernel clamps the class at 1023) between reads of two and three windows of the same geometry."""
    long_ones = [p for p in CATALOGUE if p.ws == 20]
    assert sorted(len(p.p["cons"]) for p in long_ones) == [1022, 1023, 1024, 1500] and sr.ST["ORDER_CLAMP"] == 1023
    short = []
    for i in range(12):
        R = pb.rand_lower(500 + i, 60)
        short.append(pb.Probe(f"short {i}", R, [pb.win(R, 18 * j, 18 * j + 20) for j in range(2 + i % 2)], {}, ws=20, wo=2))
    probes = short[:5] + long_ones[:2] + short[5:9] + long_ones[2:] + short[9:]
    got = launch(engines[library], probes)
    for p, g in zip(probes, got):
        r = ref_of(p.name) if p.name in BY_NAME else sr.stitch(p.p, p.k, p.ws, p.wo)
        assert g == (r.string, r.status), p.name


@pytest.mark.parametrize("library", ["product", "aids"])
def test_out_slots_and_their_guard_bytes(engines, library):
    """A slot one byte too small for the read, one the growth of a replace outgrows by one and one that holds the grown read exactly, between other reads with slots
    of exactly their final length: status 2 and nothing, or the reference's string; the other reads are what they are alone; no guard byte behind any slot
    changes (Engine.stitch checks them)."""
    slots = [p for p in CATALOGUE if p.cap is not None]
    assert [p.cap - len(p.p["read"]) for p in slots] == [-1, 0, 1]
    others = [p for p in default_class(do_trim=False) if p.p["cons"]][:4]
    probes = [others[0], slots[0], others[1], slots[1], others[2], slots[2], others[3]]
    caps = [p.cap if p.cap is not None else max(len(p.p["read"]), len(ref_of(p.name).string)) for p in probes]
    got = launch(engines[library], probes, caps)
    assert got == [(ref_of(p.name).string, ref_of(p.name).status) for p in probes]
    assert [st for _, st in got] == [0, 2, 0, 2, 0, 0, 0]


def test_a_geometry_beyond_the_slice_is_refused(engines):
    p = BY_NAME["plain three windows"]
    reads, jobs, pos, batch, res = pb.results_of([p])
    assert 2000 + 2 * 25 > sr.ST["RMAX"]
    with pytest.raises(en.EngineError):
        engines["product"].stitch(reads, jobs, pos, batch, res, 2000, 25, True)


def test_the_witnessed_bits_are_the_reachable_set(engines):
    """The union of what the kernel itself recorded over the catalogue, launched a geometry at a time: every route bit (tests/stitch_probes.py UNREACHABLE names
    the two arms that have none)."""
    seen = {"window": set(), "read": set()}
    groups = {}
    for p in CATALOGUE:
        groups.setdefault((p.ws, p.wo, p.do_trim, p.cap), []).append(p)
    for (ws, wo, trim, cap), probes in groups.items():
        with traced():
            launch(engines["aids"], probes, None if cap is None else [cap] * len(probes))
        check_witness(engines["aids"], probes, seen)
    assert seen["window"] == set(sr.WINDOW_BITS), sorted(set(sr.WINDOW_BITS) - seen["window"])
    assert seen["read"] == set(sr.READ_BITS), sorted(set(sr.READ_BITS) - seen["read"])
