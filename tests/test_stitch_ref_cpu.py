"""CPU: the plain restatement of the read re-assembly (tests/stitch_ref.py) against the oracle (oracle/cw_oracle_c.cpp cwo_stitch, cwo_ssw) on every probe of
tests/stitch_probes.py and on the random reads of tests/test_gpu_stitch.py; every probe's hand-written route against the reference's; the catalogue's cover of
the route bits; and the subtly wrong kernels (stitch_ref.MUTANTS), each caught by a named probe.  Integers and bytes throughout: every comparison is exact."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import consent_amd as ca
import oracle_lib
import stitch_probes as pb
import stitch_ref as sr
import sw_op_probes as sp
from consent_amd import engine as en
from test_oracle_stitch import stitch as oracle_stitch

CATALOGUE = pb.catalogue()
BY_NAME = {p.name: p for p in CATALOGUE}


@functools.lru_cache(maxsize=None)
def ref_of(name):
    """The reference's answer for a probe: computed once, shared, not changed."""
    p = BY_NAME[name]
    return sr.stitch(p.p, p.k, p.ws, p.wo, p.do_trim, p.cap)


def oracle_of(p, k, ws, wo, do_trim):
    """(string, status) by the oracle.  It knows no window status: a CW_WIN_OVERFLOW window is one with neither consensus nor template."""
    cons = ["" if s == sr.WIN_OVERFLOW else c for c, s in zip(p["cons"], p["status"])]
    tpls = ["" if t is None or s == sr.WIN_OVERFLOW else t for t, s in zip(p["tpls"], p["status"])]
    final, stitched = oracle_stitch(p["read"], cons, tpls, p["solid"], p["pos"], do_trim=do_trim, k=k, wsize=ws, wover=wo)
    status = 0
    if do_trim:
        ups = [i for i, c in enumerate(stitched) if c.isupper()]
        trimmed = stitched[ups[0] : ups[-1] + 1] if len(ups) > 1 else ""
        status = int(bool(trimmed) and bool(oracle_lib.oracle().cwo_drop_read(trimmed.encode(), len(trimmed))))
    return final, status


def check_alignments(r):
    for query, ref, got in r.aligns:
        want = sp.oracle(query, ref)
        assert want[: len(got)] == got, (query[:40], ref[:40], got, want)


def test_thresholds_come_from_the_header():
    assert sr.ST == {"QMAX": 2048, "RMAX": 2048, "ROWS_BYTES": 4096, "DIR_BYTES": 1 << 20, "HUGE_QMAX": 32768, "LANES": 64, "MOVE": 64, "MEM_SWEEP": 640, "ORDER_CLAMP": 1023}
    assert (sp.MATCH, sp.MISMATCH, sp.GAP_OPEN, sp.GAP_EXT) == (2, 2, 3, 1) and sp.GAP_OPEN >= sp.GAP_EXT  # the running maximum of the in-column gap needs it


def test_route_names_are_the_engines():
    band = [b for b in sr.WINDOW_BITS if b in en.STITCH_BAND]
    assert list(en.STITCH_ROUTE) + list(en.STITCH_BAND) == list(sr.WINDOW_BITS) and band == list(en.STITCH_BAND)
    assert list(en.STITCH_READ) == list(sr.READ_BITS)
    assert [v for v in en.STITCH_ROUTE.values()] == [1 << i for i in range(30)] and len(en.STITCH_FACTS) + 2 <= en.STITCH_WIT_WORDS


def test_the_reference_sweep_is_the_plain_column():
    """stitch_ref.sweep (a numpy row per column) against test_sw_op_cpu's plain Python column on the tie probes."""
    from test_sw_op_cpu import _last_column

    for q, r in sp.tie_pairs().values():
        score, rb, re_, qb, qe = sr.align(q, r)
        col = _last_column(q, r, re_)
        assert max(col) == score and col.index(score) == qe and sp.oracle(q, r)[:5] == (score, rb, re_, qb, qe)
    for q, r in sp.nothing_pairs().values():
        assert sr.align(q, r) == (0, 0, -1, 0, -1)


@pytest.mark.parametrize("g", [10, 40])
def test_the_reference_band_is_banded_best(g):
    """stitch_ref.banded_indels against sw_op_probes.banded_best and the oracle's indel totals on the planted pairs."""
    q, r = sp.planted(g)
    score, rb, re_, qb, qe, ins, dele = sp.oracle(q, r)
    rc, qc = sr.codes(r)[rb : re_ + 1], sr.codes(q)[qb : qe + 1]
    got = sr.banded_indels(rc, qc, score)
    assert got[:2] == (ins, dele) == (g, g) and got[3] == sp.bands_tried(0, g)
    assert sp.banded_best(rc, qc, got[3][-1]) >= score > sp.banded_best(rc, qc, got[3][-2])
    assert ("band_lanes" in got[2]) == (2 * got[3][-1] + 1 <= 64) and "band_doubled" in got[2]


@pytest.mark.parametrize("name", list(BY_NAME))
def test_probe(name):
    """The reference against the oracle (string, status, every alignment's numbers), and the probe's hand-written route, numbers and trace words against
    the reference's."""
    p, r = BY_NAME[name], ref_of(name)
    if p.cap is None:
        assert (r.string, r.status) == oracle_of(p.p, p.k, p.ws, p.wo, p.do_trim)
    if len(p.p["read"]) < 5000:
        check_alignments(r)
    for w, bits in p.expect.items():
        assert r.windows[w].route == bits, (w, sorted(r.windows[w].route ^ bits))
    assert r.route == p.read_route, sorted(r.route ^ p.read_route)
    for w, facts in p.facts.items():
        assert {f: r.windows[w].facts.get(f) for f in facts} == facts, w
    for w, words in p.trace.items():
        assert {i: r.windows[w].trace[i] for i in words} == words, (w, r.windows[w].trace)
    if getattr(p, "string", None) is not None:
        assert r.string == p.string
    for w in r.windows:  # a window no alignment was tried for reports no trace and no numbers
        assert (w.trace is None) == bool(w.route & {"overflow_skipped", "template_absent", "no_slice"} or not w.route), sorted(w.route)


def test_capacity_probes_differ_in_the_slot_alone():
    small, outgrown, exact = (ref_of(n) for n in ("a slot one byte smaller than the read", "a slot the growth of a replace outgrows by one", "a slot that holds the grown read exactly"))
    assert (small.string, small.status) == ("", sr.READ_CAPACITY) == (outgrown.string, outgrown.status)
    p = BY_NAME["a slot that holds the grown read exactly"]
    assert exact.status == 0 and len(exact.string) == p.cap == len(p.p["read"]) + 1
    assert (exact.string, 0) == oracle_of(p.p, p.k, p.ws, p.wo, p.do_trim)


def test_the_trim_edges_stand_where_they_say():
    kept, dropped = ref_of("10 upper-case characters of 100"), ref_of("9 upper-case characters of 91")
    assert len(kept.string) == 100 and sum(c.isupper() for c in kept.string) == 10 and kept.status == 0
    assert (dropped.string, dropped.status) == ("", sr.READ_DROPPED)
    raw = ref_of("9 upper-case characters of 91, not trimmed").string
    ups = [i for i, c in enumerate(raw) if c.isupper()]
    assert len(ups) == 9 and ups[-1] - ups[0] + 1 == 91
    assert np.float32(10) / np.float32(100) >= 0.1 > 10 / 100 - 1e-12 and float(np.float32(9) / np.float32(91)) < 0.1
    for at in (1, 64, 65):
        assert ref_of(f"the first upper-case character at {at}, not trimmed").string.index("G") == at


def test_reference_equals_oracle_on_random_reads():
    """The random specs of tests/test_gpu_stitch.py, their consensuses and solid sets a fixed result set made by the oracle."""
    import test_gpu_stitch as tg

    for seed, n, depth, kw, geom in ((101, 3, 12, dict(lo=700, hi=1500), (500, 50)), (104, 3, 10, dict(lo=600, hi=1200), (300, 30))):
        reads, jobs, pos, piles = tg.build(tg.make_reads(seed, n, depth, **kw), *geom)
        res, _ = oracle_lib.oracle_run(ca.Params(tg.K, tg.SOLID, 8, 2, 150), ca.pack_piles(piles))
        rng = random.Random(seed)
        for ri, w0, wn in jobs:
            cons = [res.consensus(w) for w in range(w0, w0 + wn)]
            for w in range(1, wn, 2):  # disagreeing overlaps, as test_stitch_overlap_reconciliation_paths makes them
                s = list(cons[w])
                for _ in range(4):
                    if len(s) > 80:
                        s[rng.randrange(5, 70)] = rng.choice("ACGT")
                cons[w] = "".join(s)
            p = dict(read=reads[ri], pos=pos[w0 : w0 + wn], cons=cons, solid=[list(res.solid_kmers(w)) for w in range(w0, w0 + wn)],
                     tpls=[piles[w][0] if piles[w] else None for w in range(w0, w0 + wn)], status=[0] * wn)
            for trim in (True, False):
                r = sr.stitch(p, tg.K, geom[0], geom[1], trim)
                assert (r.string, r.status) == oracle_of(p, tg.K, geom[0], geom[1], trim), (seed, ri, trim)
            check_alignments(r)


def test_the_catalogue_covers_every_route_bit():
    windows, reads = set(), set()
    for name in BY_NAME:
        r = ref_of(name)
        reads |= r.route
        for w in r.windows:
            windows |= w.route
    assert windows == set(sr.WINDOW_BITS) and reads == set(sr.READ_BITS)
    assert set(pb.UNREACHABLE) == {"size_al beyond CW_ST_RMAX", "overlap beyond CW_ST_RMAX in the last launch"}
    hand = set().union(*(p.expect[w] for p in CATALOGUE for w in p.expect))
    assert hand == set(sr.WINDOW_BITS) and set().union(*(p.read_route for p in CATALOGUE)) == set(sr.READ_BITS)  # by the hand-written routes alone, too


def test_no_overlap_outgrows_a_slice():
    """UNREACHABLE's second entry: 300 random reads of two to five windows whose starts do not descend, consensuses with inserts of up to 300 letters (ten windows'
    length), some windows on their template, at window sizes of 20-59 and overlaps of 0-11: no overlap exceeds window_size + 2 * window_overlap."""
    rng = random.Random(5)
    most = -10 ** 9
    for case in range(300):
        ws, wo = rng.randrange(20, 60), rng.randrange(0, 12)
        n = rng.randrange(2, 6)
        R = pb.rand_lower(1000 + case, 60 * n + 200)
        wins, first = [], rng.randrange(0, 30)
        for i in range(n):
            body = R[first : min(len(R), first + rng.randrange(pb.K, ws + 2 * wo))].upper()
            x = rng.randrange(0, len(body))
            cons = body[:x] + pb.rand_lower(case * 7 + i, rng.choice([0, 0, 5, 60, 300])).upper() + body[x:]
            wins.append((first, first + ws - 1, "ACG" if rng.random() < 0.2 else cons, (), cons, 0))
            first += rng.randrange(0, ws)
        r = sr.stitch(pb.Probe("search", R, wins, {}, ws=ws, wo=wo).p, pb.K, ws, wo)
        most = max([most] + [w.facts["overlap"] - (ws + 2 * wo) for w in r.windows if "overlap" in w.facts])
    assert most == 0, most  # reached exactly, never passed


@pytest.mark.parametrize("mutant", list(pb.MUTANT_CAUGHT_BY))
def test_mutant_is_caught(mutant):
    """A kernel wrong in this one decision would fail the named probe: its final string or status differs from the reference's."""
    name = pb.MUTANT_CAUGHT_BY[mutant]
    p, good = BY_NAME[name], ref_of(name)
    bad = sr.stitch(p.p, p.k, p.ws, p.wo, p.do_trim, p.cap, mut=[mutant])
    assert (bad.string, bad.status) != (good.string, good.status), name


def test_the_two_switches_that_change_nothing():
    assert set(pb.MUTANT_CAUGHT_BY) | set(pb.EQUIVALENT_MUTANTS) == set(sr.MUTANTS) and not set(pb.MUTANT_CAUGHT_BY) & set(pb.EQUIVALENT_MUTANTS)
    for mutant in pb.EQUIVALENT_MUTANTS:
        for name, p in BY_NAME.items():
            if len(p.p["read"]) < 1000:
                bad, good = sr.stitch(p.p, p.k, p.ws, p.wo, p.do_trim, p.cap, mut=[mutant]), ref_of(name)
                assert (bad.string, bad.status, [w.trace for w in bad.windows]) == (good.string, good.status, [w.trace for w in good.windows]), (mutant, name)
    # no float in [0.1, 0.1f): the floats around 0.1f compare alike with the double and with the float
    f = np.float32(0.1)
    for r in (np.nextafter(f, np.float32(0)), f, np.nextafter(f, np.float32(1))):
        assert (float(r) < 0.1) == bool(r < f)
    for ws, wo, al_pos in ((100, 10, 80), (500, 50, 0)):  # on the slice's edge the clipped size is the full size
        tot = al_pos + ws + 2 * wo
        assert tot - al_pos == ws + 2 * wo
