"""The chain kernel's chain and segment cuts as numbers.  Every other GPU test sees cw_chain_kernel through the final consensus string, which a wrong tie,
a cut moved by one anchor or a wrong choice of the first max_msa members often spells just the same.  Here every probe of tests/chain_probes.py -- one
window, alone in its batch, aimed at one edge of the kernel's scoring routes, its early stop, its tie rules or its flush -- is run on the product library
and on the test-aid library.  Each run is compared with the oracle (status, consensus, solid set: that locates a failure) and with the plain reference
of chain_probes.py, exactly: the window's segment count, every POA task's segment and members in order, the lengths of the segments the kernel writes
itself (Engine.segments), the kernel's own counters (Engine.profile), and on the test-aid library the route witness (Engine.chain_route), which must be
the probe's hand-written route.  Then the reference's task segments go through Engine.poa as groups: cw_poa_tasks_kernel (cw_poa_op.h) calls the routing
rule the flush calls (cw_poa_route) and must send them to the same tiers, and each consensus must be the oracle's POA of its members."""
import os

import numpy as np
import pytest

import consent_amd as ca
import oracle_lib
from chain_probes import PROBES, pieces
from consent_amd import engine
from consent_amd.engine import CHAIN_ROUTE, INDEX_ROUTE, route_names

pytestmark = pytest.mark.gpu
THREADS = min(16, os.cpu_count() or 1)


@pytest.fixture(scope="module")
def engines():
    cache = {}  # at most four engines alive, as in test_gpu_index_counts.py; the pair of long templates gets its configured engine

    def get(which, prm, configure=None):
        key = (which, prm, configure)
        if key in cache:
            cache[key] = cache.pop(key)
        else:
            while len(cache) >= 4:
                cache.pop(next(iter(cache))).close()
            cache[key] = ca.Engine(ca.Params(*prm))
            if configure:
                cache[key].configure(configure)
        want = engine.AIDS_LIB if which == "aids" else engine.lib_path()
        assert cache[key].lib._name == want, (cache[key].lib._name, want)
        return cache[key]

    yield get
    for e in cache.values():
        e.close()


_EXP = {}


def expected(probe):
    """The oracle's window, and the oracle's POA of every task segment of the reference: once per probe."""
    if probe.name not in _EXP:
        exp, _ = oracle_lib.oracle_run(ca.Params(*probe.prm), probe.hb, threads=THREADS)
        groups = [pieces(probe.pile, mem) for _, mem in probe.ref.tasks]
        _EXP[probe.name] = (exp, groups, [oracle_lib.oracle_poa(g) for g in groups])
    return _EXP[probe.name]


def tiers_of(ctr):
    """Tasks per tier of the last run: S (no list: by difference), then the lists Q, M1, M2, L, 4, H."""
    lists = [int(x) for x in ctr[6:12]]
    return [int(ctr[0]) - sum(lists)] + lists


def run_and_compare(e, probe):
    exp, groups, group_cons = expected(probe)
    ref = probe.ref
    got = e.run(probe.hb)
    assert int(got.status[0]) != ca.WIN_OVERFLOW, f"{probe}: stopped, why {int(e.win_info(1)[0, 15])}"
    assert int(got.status[0]) == int(exp.status[0]), f"{probe}: status {got.status[0]} != {exp.status[0]}"
    assert got.consensus(0) == exp.consensus(0), f"{probe}: consensus differs from the oracle's"
    assert np.array_equal(got.solid_kmers(0), exp.solid_kmers(0)), f"{probe}: solid set differs from the oracle's"
    # the segmentation
    n_segs, seg_len, tasks = e.segments(0)
    assert n_segs == len(ref.segments), f"{probe}: {n_segs} segments, the reference has {len(ref.segments)} (chain of {len(ref.chain)})"
    by_seg = {}
    for seg, n, longest, members in tasks:
        assert seg not in by_seg, f"{probe}: two task records for segment {seg}"
        by_seg[seg] = (n, longest, members)
    assert sorted(by_seg) == [i for i, _ in ref.tasks], f"{probe}: task records for segments {sorted(by_seg)}, the reference's tasks are {[i for i, _ in ref.tasks]}"
    for i, mem in ref.tasks:
        assert by_seg[i] == (len(mem), max(l for _, _, l in mem), mem), f"{probe}: segment {i}: {by_seg[i]} against {mem}"
    for i, (cls, mem) in enumerate(ref.segments):
        if cls != "task":  # (a task's seg_len is the POA's output)
            assert int(seg_len[i]) == (mem[0][2] if mem else 0), f"{probe}: {cls} segment {i} has length {int(seg_len[i])}, members {mem}"
    # the kernel's counters
    ctr, prof = e.profile()
    assert [int(prof[i]) for i in (42, 43, 44)] == [ref.A, probe.n_dirty, 1], f"{probe}: anchors, dirty sequences, windows {prof[42:45]}"
    assert tuple(int(prof[i]) for i in (50, 51, 52, 53)) == probe.counters, f"{probe}: fix windows, rows, bad masks, slow {prof[50:54]}, designed {probe.counters}"
    assert (int(ctr[0]), int(ctr[1])) == (len(ref.tasks), ref.n_members), f"{probe}: {ctr[0]} tasks of {ctr[1]} members, the reference {len(ref.tasks)} of {ref.n_members}"
    routes = (int(prof[engine.CHAIN_ROUTE_SLOT]), int(prof[engine.INDEX_ROUTE_SLOT]))
    # the operator routes by the same rule: the same tasks as groups, on the same engine (by_anchor segments stay out: the operator aligns them)
    if groups:
        window_tiers = tiers_of(ctr)
        res = e.poa(groups)
        assert tiers_of(e.profile()[0]) == window_tiers, f"{probe}: the operator routed {tiers_of(e.profile()[0])}, the chain kernel {window_tiers} (S, Q, M1, M2, L, -, H)"
        for g, cons in enumerate(group_cons):
            assert int(res.status[g]) == ca.WIN_CONSENSUS and res.consensus(g) == cons, f"{probe}: group {g} (segment {ref.tasks[g][0]}) differs from the oracle's POA"
    return routes


@pytest.mark.parametrize("probe", PROBES, ids=repr)
def test_chain_on_the_product_library(probe, engines):
    chain_route, index_route = run_and_compare(engines("product", probe.prm, probe.configure), probe)
    assert chain_route == 0 and index_route == 0  # no witness in the product's kernels


@pytest.mark.parametrize("probe", PROBES, ids=repr)
def test_chain_and_route_on_the_test_aid_library(probe, engines, aids):
    chain_route, index_route = run_and_compare(engines("aids", probe.prm, probe.configure), probe)
    assert chain_route == probe.route, f"{probe}: went {route_names(chain_route, CHAIN_ROUTE)}, designed for {probe.route_names}"
    assert bool(index_route & INDEX_ROUTE["use_bits"]) == probe.use_bits, f"{probe}: index route {route_names(index_route)}"
